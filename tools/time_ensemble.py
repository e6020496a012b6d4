"""Time posterior ensembles on the GPU: one K-member pass against K one-member passes, and ``pdse_ensemble_stats`` alone.
Run on the GPU machine only:

    python tools/time_ensemble.py [--members 1 4 8 16] [--seconds 4] [--runs 5] [--out profiles/ensemble_timing.txt]

1. A B = 1 file of ``--seconds`` through ``ComplexDDPMTrainer.enhance(wav, x_T, members=K)`` for every K, against K sequential
   ``enhance(wav, x_T[k])`` calls of the same trainer (members=1: the one-file pass, replayed from its hipGraph once the geometry
   came back, as the file loop runs it) in the same session.  One untimed call of each first (plan, graph capture); then the
   median of ``--runs`` wall-clock times around synchronised calls, with the lowest and the highest.
2. The bandwidth of ``pdse_ensemble_stats`` alone at B = 32, T = 401, K = 8: hipEvents around 20 calls, median of ``--runs``;
   bytes = (K + 1.5) n 4 with n = B 2 T 161.

Prints one line per figure and a ``RESULT`` json line; ``--out`` appends them to a file."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch

    import __graft_entry__ as ge

    ge.build()
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    synth = importlib.import_module("prior-diffuse_amd.synth")
    trainer = importlib.import_module("prior-diffuse_amd.trainer")
    ops = importlib.import_module("prior-diffuse_amd.ops")
    ns = argparse.Namespace
    lines = []

    def report(name, unit, vals, **extra):
        res = dict(name=name, unit=unit, median=round(statistics.median(vals), 4), min=round(min(vals), 4), max=round(max(vals), 4),
                   runs=len(vals), **extra)
        lines.append("%-72s %9.3f %s  (%.3f .. %.3f)" % (name, res["median"], unit, res["min"], res["max"]))
        lines.append("RESULT " + json.dumps(res))
        print(lines[-2], flush=True)
        print(lines[-1], flush=True)

    tr = trainer.ComplexDDPMTrainer(
        ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav="unused"),
        ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
        device="cuda:0", prior_state_dict=synth.make_state_dict("GCRN"), ddpm_state_dict=synth.make_state_dict("DiffUNet1"))
    n = int(round(args.seconds * 16000))
    T = 1 + n // 160
    wav = torch.as_tensor(synth.speechlike(1, n, 100)[0], dtype=torch.float32)[None].cuda()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return ms

    with torch.no_grad():
        for K in args.members:
            x_T = torch.randn(K, 1, 2, T, 161, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(K))
            tr.enhance(wav, x_T[0])                                        # the one-member geometry met once: replayed from here on
            seq = timed(lambda: [tr.enhance(wav, x_T[k]) for k in range(K)])
            one = timed(lambda: tr.enhance(wav, x_T, members=K))
            report("B=1 %.0f s: %2d sequential members=1 passes" % (args.seconds, K), "ms", seq, members=K)
            report("B=1 %.0f s: one members=%d pass" % (args.seconds, K), "ms", one, members=K)
        B, T2, K = 32, 401, 8
        x = torch.randn(K * B, 2, T2, 161, device="cuda:0")
        import numpy as np

        lib = importlib.import_module("prior-diffuse_amd._lib")
        frames_h = np.full(B, T2, dtype=np.int32)
        frames = torch.from_numpy(frames_h).cuda()
        mean, spread = torch.empty(B, 2, T2, 161, device="cuda:0"), torch.empty(B, T2, 161, device="cuda:0")
        partial = torch.empty(B * lib.ENSEMBLE_BLOCKS * (K + 2), dtype=torch.float64, device="cuda:0")
        per_utt, per_member = torch.empty(B, 2, dtype=torch.float64, device="cuda:0"), torch.empty(K, B, dtype=torch.float64, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream

        def call():     # the entry point itself, on buffers made once: no allocation and no copy between the launches
            lib.ensemble_stats(x.data_ptr(), mean.data_ptr(), spread.data_ptr(), frames_h.ctypes.data, frames.data_ptr(), partial.data_ptr(),
                               per_utt.data_ptr(), per_member.data_ptr(), K, B, T2, 161, stream)

        call()
        torch.cuda.synchronize()
        assert torch.equal(mean, ops.ensemble_stats(x, K, [T2] * B)["mean"])
        ms = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / 20)
        nbytes = (K + 1.5) * B * 2 * T2 * 161 * 4
        report("pdse_ensemble_stats alone, B=32 T=401 K=8 (%.1f MB moved)" % (nbytes / 1e6), "ms per call", ms)
        report("pdse_ensemble_stats alone, B=32 T=401 K=8", "GB/s", [nbytes / (m * 1e-3) / 1e9 for m in ms])
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
