"""Time the B = 1 file loop, ``ComplexDDPMTrainer.generate_wav``, on directories of wav files at a given sample rate: what a
file costs from the wav read (decode, mono mix, conversion to 16 kHz) to the written result.  16 synthetic 4 s files per rate,
one untimed run (weights, plan, graph capture), then three timed runs; prints the median ms per file with the lowest and the
highest run.  Only the public interface is used, so the same script times any checkout of the project:

    python tools/time_file_loop.py [--rates 16000 44100 48000] [--root OTHER_CHECKOUT] [--files 16] [--seconds 4] [--runs 3]

Lines of several invocations (say, this commit and its parent, alternating) are collected in profiles/wav_frontend_timing.txt.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", type=int, nargs="+", default=[16000, 44100, 48000])
    ap.add_argument("--root", default=HERE, help="the checkout to time (default: the one this script lies in)")
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import numpy as np
    import torch

    import __graft_entry__ as ge

    ge.build()
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    synth = importlib.import_module("prior-diffuse_amd.synth")
    wavio = importlib.import_module("prior-diffuse_amd.wavio")
    trainer = importlib.import_module("prior-diffuse_amd.trainer")
    ns = argparse.Namespace
    label = args.label or os.path.basename(root)
    work = tempfile.mkdtemp(prefix="file_loop_")
    try:
        tr = trainer.ComplexDDPMTrainer(
            ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav=os.path.join(work, "out")),
            ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
            device="cuda:0", prior_state_dict=synth.make_state_dict("GCRN"), ddpm_state_dict=synth.make_state_dict("DiffUNet1"))
        for rate in args.rates:
            src = os.path.join(work, "in_%d" % rate)
            os.makedirs(src)
            n = int(round(args.seconds * rate))
            for i in range(args.files):
                wavio.write_wav(os.path.join(src, "f%02d.wav" % i), synth.speechlike(1, n, 100 + i)[0], rate)
            torch.manual_seed(1)
            written = tr.generate_wav(load_pre_train=False, data_path=src)       # untimed: plan, graph capture, tap table
            assert len(written) == args.files
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                tr.generate_wav(load_pre_train=False, data_path=src)
                torch.cuda.synchronize()
                ms.append(1e3 * (time.perf_counter() - t0) / args.files)
            res = {"label": label, "rate": rate, "files": args.files, "seconds_per_file": args.seconds,
                   "ms_per_file_median": round(statistics.median(ms), 3), "ms_per_file_min": round(min(ms), 3),
                   "ms_per_file_max": round(max(ms), 3), "runs": args.runs}
            print("%-10s %6d Hz: %8.3f ms per file (%.3f .. %.3f over %d runs of %d files of %.1f s)" % (
                label, rate, res["ms_per_file_median"], res["ms_per_file_min"], res["ms_per_file_max"], args.runs, args.files,
                args.seconds), flush=True)
            print("RESULT " + json.dumps(res), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
