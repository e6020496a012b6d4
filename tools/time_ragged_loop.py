"""Time the file loop on a directory of files of DIFFERENT lengths, one file per pass against exact ragged batches:
``ComplexDDPMTrainer.generate_wav(batch=1)`` and ``generate_wav(batch=N)`` on the same synthetic directory (64 files, lengths
spread evenly over 2 - 6 s, 16 kHz), in the same process, alternating.  One untimed run of each (weights, plans, graph capture),
then ``--runs`` timed runs of each; prints the median ms per file with the lowest and the highest run, the padding waste of the
batched loop (padded frames / own frames) and whether both loops wrote the same bytes.

    python tools/time_ragged_loop.py [--files 64] [--batch 32] [--runs 3] [--out profiles/ragged_file_loop_timing.txt]
    python tools/time_ragged_loop.py --prior aia_complex_trans_ri --batch 8 --out profiles/ragged_aia_timing.txt

``--prior`` names the prior network (default GCRN); the DB-AIAT priors are built with ``masked_prior=True``, without which their
batched loop is refused.
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
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=2.0)
    ap.add_argument("--max-seconds", type=float, default=6.0)
    ap.add_argument("--shared", action="store_true",
                    help="build both trainers with exclusive=False (the kernels that do not depend on the batch size: the two loops then "
                         "write the same bytes); default: the trainers a user gets, whose one-file loop takes the persistent small-batch LSTM")
    ap.add_argument("--prior", default="GCRN", choices=("GCRN", "DiffUNet", "aia_complex_trans_ri", "dual_aia_trans_merge_crm"),
                    help="the prior network; the DB-AIAT priors run their batches on the length-masked kernels (masked_prior=True)")
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch

    import __graft_entry__ as ge

    ge.build()
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    synth = importlib.import_module("prior-diffuse_amd.synth")
    wavio = importlib.import_module("prior-diffuse_amd.wavio")
    trainer = importlib.import_module("prior-diffuse_amd.trainer")
    raggedplan = importlib.import_module("prior-diffuse_amd.raggedplan")
    ns = argparse.Namespace
    work = tempfile.mkdtemp(prefix="ragged_loop_")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        src = os.path.join(work, "in")
        os.makedirs(src)
        # lengths spread evenly over the range, in an order that is not sorted (a seeded shuffle): the loop has to sort them itself
        lens = np.linspace(args.min_seconds * 16000, args.max_seconds * 16000, args.files).astype(int)
        np.random.RandomState(3).shuffle(lens)
        for i, n in enumerate(lens):
            wavio.write_wav(os.path.join(src, "f%03d.wav" % i), synth.speechlike(1, int(n), 100 + i)[0], 16000)
        waste = sum(raggedplan.padding_waste(lens[lo:hi], args.batch) * sum(1 + int(n) // 160 for n in lens[lo:hi])
                    for lo, hi in raggedplan.windows(len(lens), args.batch)) / sum(1 + int(n) // 160 for n in lens)
        trs = {}
        masked = ("aia_complex_trans_ri", "dual_aia_trans_merge_crm")
        for batch in (1, args.batch):
            trs[batch] = trainer.ComplexDDPMTrainer(
                ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav=os.path.join(work, "out%d" % batch)),
                ns(model=ns(name=args.prior), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
                device="cuda:0", prior_state_dict=synth.make_state_dict(args.prior), ddpm_state_dict=synth.make_state_dict("DiffUNet1"),
                exclusive=False if args.shared else None, masked_prior=args.prior in masked)
            torch.manual_seed(1)
            written = trs[batch].generate_wav(load_pre_train=False, data_path=src, batch=batch)     # untimed
            assert len(written) == args.files
        torch.cuda.synchronize()
        same = all(open(os.path.join(work, "out1", f), "rb").read() == open(os.path.join(work, "out%d" % args.batch, f), "rb").read()
                   for f in sorted(os.listdir(os.path.join(work, "out1"))))
        ms = {1: [], args.batch: []}
        for _ in range(args.runs):
            for batch in (1, args.batch):
                t0 = time.perf_counter()
                trs[batch].generate_wav(load_pre_train=False, data_path=src, batch=batch)
                torch.cuda.synchronize()
                ms[batch].append(1e3 * (time.perf_counter() - t0) / args.files)
        res = {"prior": args.prior, "files": args.files, "seconds": [args.min_seconds, args.max_seconds], "runs": args.runs, "batch": args.batch,
               "padding_waste": round(waste, 4), "same_bytes": bool(same), "exclusive": not args.shared}
        for batch in (1, args.batch):
            res["ms_per_file_batch%d" % batch] = [round(statistics.median(ms[batch]), 3), round(min(ms[batch]), 3), round(max(ms[batch]), 3)]
            say("%s generate_wav(batch=%-2d): %8.3f ms per file (%.3f .. %.3f over %d runs of %d files of %.0f - %.0f s)" % (
                args.prior, batch, statistics.median(ms[batch]), min(ms[batch]), max(ms[batch]), args.runs, args.files, args.min_seconds, args.max_seconds))
        say("padding waste of batch=%d: %.3f padded frames per own frame; written files byte-identical to batch=1: %s (trainers %s)" % (
            args.batch, waste, same, "exclusive=False" if args.shared else
            "as a user gets them" + (": batch=1 on the persistent small-batch LSTM" if args.prior == "GCRN" else "")))
        say("RESULT " + json.dumps(res))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
