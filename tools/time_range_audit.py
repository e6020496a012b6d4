"""Time the range audit of the f16x2 window (csrc/range.hip) at the bench geometry, B = 32 x 4 s (T = 401), GCRN prior, 6 steps,
in one process (hipEvents, warm-up, median of 20): the sequential ``SamplerPipeline.enhance`` pass un-audited and audited (eager
and hipGraph replay), the accumulate launch of one step on its own, and the kernel alone on the largest plane tensor of the
plan (bytes read: the hi plane's logical box) and on the largest fp32 tensor.  Prints the paragraph that
profiles/range_audit_timing.txt holds.

    python tools/time_range_audit.py [--out FILE]
"""
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup=3, reps=20):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    import torch

    import __graft_entry__ as ge

    ge.build()
    L = importlib.import_module("prior-diffuse_amd._lib")
    RA = importlib.import_module("prior-diffuse_amd.rangeaudit")
    synth = importlib.import_module("prior-diffuse_amd.synth")
    P = importlib.import_module("prior-diffuse_amd.pipeline").SamplerPipeline
    dev = "cuda:0"
    B, L_ = 32, 64000
    gs, ds = synth.make_state_dict("GCRN"), synth.make_state_dict("DiffUNet1")
    wav, x_T = synth.synthetic_waveforms(B, L_, seed=1234)
    wav, x_T = wav.to(dev), x_T.to(dev)
    lines = ["range audit (csrc/range.hip), hipEvent times in ms: median [min .. max] of 20, B = 32, L = 64000 (T = 401), GCRN, 6 steps"]
    pipes = {}
    for tag, kw in (("un-audited", {}), ("audited", dict(audit=True))):
        pipes[tag] = p = P(dev, "GCRN", gs, ds, B, L_=L_, exclusive=True, **kw)
        for mode, graph in (("eager", False), ("graph", True)):
            med, lo, hi = timed(lambda: p.run(graph=graph) if graph else p.run())
            lines.append("  sequential pass, %-10s %-5s  %8.3f [%8.3f .. %8.3f]   %d launches" % (tag, mode, med, lo, hi, len(p.descs)))
        p.stft.wav.copy_(wav)
        p.xT_in.copy_(x_T)
        p.stft.lens.fill_(L_)
        p.run()
        p.check()
    aud = pipes["audited"]
    rep = aud.range_report()
    lines.append("  report of that pass: %d rows, ok = %s, worst: %r" % (len(rep), rep.ok, rep.worst()))
    b, e = aud.ranges["step0"]
    med, lo, hi = timed(lambda: aud.plan.run_range(e - 1, e, torch.cuda.current_stream().cuda_stream))
    lines.append("  accumulate launch of one step (%d tensors)   %8.3f [%8.3f .. %8.3f]" % (len(aud.eps.audited()), med, lo, hi))
    out = torch.zeros(1, 32, dtype=torch.int32, device=dev)
    for what, pick in (("largest plane tensor", L.RANGE_F16HI), ("largest fp32 tensor", L.RANGE_F32)):
        name, t, kind, ex, box = max((a for a in aud.eps.audited() + aud.prior.audited() if a[2] == pick), key=lambda a: a[1].numel())
        row = RA.make_row(t, kind, ex, box, 0)
        tab = torch.from_numpy(RA.table_of([row])).to(dev)
        d = L.RangeDesc()
        d.rows, d.out, d.nrows, d.out_rows, d.mode = tab.data_ptr(), out.data_ptr(), 1, 1, L.RANGE_ACCUMULATE
        nbytes = row.n * (2 if pick == L.RANGE_F16HI else 4)
        for blocks in (RA.work_blocks([row]), 256, 1024, 2048):
            d.blocks = blocks
            plan = L.Plan(dev)                  # recorded: the table is validated once, a run is the launch alone
            plan.add(d)
            med, lo, hi = timed(lambda: plan.run(torch.cuda.current_stream().cuda_stream), warmup=5, reps=30)
            lines.append("  kernel alone, %s %s (%.1f MB read), %4d workgroups  %7.4f [%7.4f .. %7.4f]  %7.1f GB/s" % (
                what, name, nbytes / 1e6, blocks, med, lo, hi, nbytes / med / 1e6))
    text = "\n".join(lines) + "\n"
    print(text)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
