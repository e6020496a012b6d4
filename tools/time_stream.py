"""Time utterances in flight through the trainer's public surface (``ComplexDDPMTrainer.enhance_stream``,
``generate_wav(inflight=N)``), on the GPU, and write the figures to profiles/stream_timing.txt:

  (a) ms per file of ``generate_wav`` on a directory of 64 synthetic 4 s files (16 kHz), inflight 1 and inflight 3;
  (b) ms per B = 32 x 4 s batch through ``enhance_stream(inflight=3)``, beside ``PipelinedSampler(depth=3, by_batch=True)``
      driven directly (submit / drain, as bench.py drives it) in the same process;
  (c) what the verdict costs: a ``SamplerPipeline(verdict=True)`` pass against a ``verdict=False`` pass, sequential, replayed
      from their hipGraphs.

Every figure is the median of ``--runs`` (at least 5) timed repeats after one untimed repeat, with the lowest and the highest
repeat; the arms of a comparison alternate within one process.  A host clock around work that ends in a device synchronise.

    python tools/time_stream.py [--files 64] [--seconds 4] [--batches 12] [--runs 5] [--out profiles/stream_timing.txt]

The yardstick of (a) is tools/time_file_loop.py of the parent commit, run in the same session (--rates 16000 --files 64 --runs 5).
"""
import argparse
import importlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batches", type=int, default=12, help="batches per timed repeat of (b); passes per repeat of (c)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "stream_timing.txt"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: at least 5 repeats")
    sys.path.insert(0, HERE)
    import torch

    import __graft_entry__ as ge

    ge.build()
    if not torch.cuda.is_available():
        raise SystemExit("time_stream.py needs the GPU: a timing taken elsewhere says nothing")
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    synth = importlib.import_module("prior-diffuse_amd.synth")
    wavio = importlib.import_module("prior-diffuse_amd.wavio")
    trainer = importlib.import_module("prior-diffuse_amd.trainer")
    pipeline = importlib.import_module("prior-diffuse_amd.pipeline")
    ns = argparse.Namespace
    dev = "cuda:0"
    gs, ds = synth.make_state_dict("GCRN"), synth.make_state_dict("DiffUNet1")
    lines, results = [], []

    def report(name, what, ms, unit):
        s = summary(ms)
        results.append(dict(s, name=name, unit=unit))
        lines.append("%-34s %9.3f %s  (%.3f .. %.3f over %d repeats)  %s" % (name, s["median"], unit, s["min"], s["max"], s["runs"], what))
        print(lines[-1], flush=True)
        return s

    def timed(fn, per):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / per

    work = tempfile.mkdtemp(prefix="stream_timing_")
    try:
        def make_trainer():
            return trainer.ComplexDDPMTrainer(
                ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav=os.path.join(work, "out")),
                ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
                device=dev, prior_state_dict=gs, ddpm_state_dict=ds)

        # ---- (a) the file loop -------------------------------------------------------------------------------------
        src = os.path.join(work, "in")
        os.makedirs(src)
        n = int(round(args.seconds * 16000))
        for i in range(args.files):
            wavio.write_wav(os.path.join(src, "f%02d.wav" % i), synth.speechlike(1, n, 100 + i)[0], 16000)
        tr = make_trainer()
        arms = {1: [], args.inflight: []}
        for rep in range(args.runs + 1):
            for k in arms:                                              # alternating; repeat 0 is the warm-up of both
                torch.manual_seed(1)
                ms = timed(lambda: tr.generate_wav(load_pre_train=False, data_path=src, inflight=k), args.files)
                if rep:
                    arms[k].append(ms)
        what = "%d files of %.1f s, 16 kHz, generate_wav" % (args.files, args.seconds)
        a1 = report("(a) file loop, inflight=1", what, arms[1], "ms per file")
        a3 = report("(a) file loop, inflight=%d" % args.inflight, what, arms[args.inflight], "ms per file")
        del tr
        torch.cuda.empty_cache()

        # ---- (b) batches in flight ---------------------------------------------------------------------------------
        B, L_ = args.batch, n
        wav, x_T = synth.synthetic_waveforms(B, L_, seed=1234)
        wav, x_T = wav.to(dev), x_T.to(dev)
        tr = make_trainer()
        direct = pipeline.PipelinedSampler(dev, "GCRN", gs, ds, B, L_, depth=args.inflight, by_batch=True, graph=True, fast_sampling=True)

        def through_trainer():
            for _ in tr.enhance_stream(((wav, x_T) for _ in range(args.batches)), inflight=args.inflight):
                pass

        def directly():
            for _ in range(args.batches):
                direct.submit(wav, x_T)
            direct.drain()

        arms = {"stream": [], "direct": []}
        for rep in range(args.runs + 2):                                # two warm-ups: a slot replays from its second visit on
            for name, fn in (("stream", through_trainer), ("direct", directly)):
                ms = timed(fn, args.batches)
                if rep > 1:
                    arms[name].append(ms)
        what = "%d batches of B = %d x %.1f s per repeat" % (args.batches, B, args.seconds)
        b_s = report("(b) enhance_stream(inflight=%d)" % args.inflight, what + ", verified, results cloned", arms["stream"], "ms per batch")
        b_d = report("(b) PipelinedSampler direct", what + ", submit / drain, unverified", arms["direct"], "ms per batch")
        del tr, direct
        torch.cuda.empty_cache()

        # ---- (c) the verdict ---------------------------------------------------------------------------------------
        pipes = {v: pipeline.SamplerPipeline(dev, "GCRN", gs, ds, B, L_=L_, verdict=v) for v in (False, True)}
        arms = {False: [], True: []}

        def passes(p):
            for _ in range(args.batches):
                p.enhance(wav, x_T, graph=True)

        for rep in range(args.runs + 1):
            for v, p in pipes.items():
                ms = timed(lambda: passes(p), args.batches)
                if rep:
                    arms[v].append(ms)
        what = "B = %d x %.1f s, sequential graph replays" % (B, args.seconds)
        c0 = report("(c) pass, verdict=False", what, arms[False], "ms per pass")
        c1 = report("(c) pass, verdict=True", what, arms[True], "ms per pass")
        lines.append("(c) verdict cost: %+.3f ms per pass (medians); spread of the plain pass %.3f ms" % (
            c1["median"] - c0["median"], c0["max"] - c0["min"]))
        lines.append("(a) inflight=%d against inflight=1: %+.3f ms per file (medians); spreads %.3f and %.3f ms" % (
            args.inflight, a3["median"] - a1["median"], a1["max"] - a1["min"], a3["max"] - a3["min"]))
        lines.append("(b) enhance_stream against the direct sampler: %+.3f ms per batch (medians); spreads %.3f and %.3f ms" % (
            b_s["median"] - b_d["median"], b_s["max"] - b_s["min"], b_d["max"] - b_d["min"]))
        for ln in lines[-3:]:
            print(ln, flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/time_stream.py --files %d --seconds %g --batch %d --batches %d --runs %d --inflight %d\n" % (
            args.files, args.seconds, args.batch, args.batches, args.runs, args.inflight))
        f.write("\n".join(lines) + "\n")
        for r in results:
            f.write("RESULT " + json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
