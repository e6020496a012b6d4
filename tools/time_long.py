"""Timing of the windowed pass over long recordings on the GPU box -> profiles/long_timing.txt.

    python tools/time_long.py --out profiles/long_timing.txt [--parent DIR] [--seconds 60] [--windows 2048 4096] [--runs 5]

Every figure: ``--runs`` (>= 5) timed passes after one untimed pass, each between two device synchronisations, median with min .. max.
  (a) one ``--seconds`` file at B = 1 as ONE whole-file plan (exclusive=False: the kernels the windowed pass takes), and with
      window=W for every W of ``--windows``, in ms per file, against the share of frames recomputed, W / (W - H_left - H_right);
      the host side of a window and step - two gathers, one run_range, one scatter - is timed apart: the gather / scatter launches
      alone at their achieved bandwidth, and the same pass with an empty plan range in place of the network
  (b) the activation bytes of the whole-file plan, of the window plan and of the windowed pass's whole-file side
  (c) the longest recording a whole-file plan can record, by arithmetic: (free device memory as the allocator reports it) /
      (activation bytes per frame of the plan of (a)); no allocation is attempted.  Beside it a ``--long-seconds`` recording,
      several times (a)'s length, through window=W
  (d) with ``--parent DIR`` (a built checkout of the parent commit): this commit against its parent in one session, in child
      processes that alternate parent / this commit, ``--rounds`` each - the whole-file plan of (a), the default file loop
      (generate_wav over ``--files`` files of 4 s) and bench.py.  The criterion: this commit's median inside the parent's own
      min .. max.
A child (``--worker whole|fileloop --root DIR``) imports the package from DIR and prints its timings as one JSON line; it uses
nothing that the parent commit lacks."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _timed(torch, fn, runs):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def worker(args):
    """One arm of (d) on the checkout ``args.root``: prints {"ms": [...]}."""
    sys.path.insert(0, args.root)
    os.chdir(args.root)
    import torch

    import __graft_entry__ as ge

    ge.build()
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    synth = importlib.import_module("prior-diffuse_amd.synth")
    dev = "cuda:0"
    gs, ds = synth.make_state_dict("GCRN"), synth.make_state_dict("DiffUNet1")
    if args.worker == "whole":
        pipeline = importlib.import_module("prior-diffuse_amd.pipeline")
        L_ = int(args.seconds * 16000) // 160 * 160
        wav, x_T = synth.synthetic_waveforms(1, L_, seed=7)
        wav, x_T = wav.to(dev), x_T.to(dev)
        pipe = pipeline.SamplerPipeline(dev, "GCRN", gs, ds, 1, L_=L_, exclusive=False)
        ms = _timed(torch, lambda: pipe.enhance(wav, x_T), args.runs)
        pipe.check()
    else:
        wavio = importlib.import_module("prior-diffuse_amd.wavio")
        trainer = importlib.import_module("prior-diffuse_amd.trainer")
        ns = argparse.Namespace
        work = tempfile.mkdtemp(prefix="long_timing_")
        src = os.path.join(work, "in")
        os.makedirs(src)
        for i in range(args.files):
            wavio.write_wav(os.path.join(src, "f%02d.wav" % i), synth.speechlike(1, 4 * 16000, 100 + i)[0], 16000)
        tr = trainer.ComplexDDPMTrainer(
            ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav=os.path.join(work, "out")),
            ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
            device=dev, prior_state_dict=gs, ddpm_state_dict=ds)

        def loop():
            torch.manual_seed(1)
            tr.generate_wav(load_pre_train=False, data_path=src)

        ms = [m / args.files for m in _timed(torch, loop, args.runs)]
    print("LONG_TIMING " + json.dumps({"ms": ms}), flush=True)


def child(root, what, args):
    """Timings of one child process on the checkout ``root``: a worker of this script, or bench.py's ms_per_step."""
    if what == "bench":
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5"]
    else:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", what, "--root", root, "--runs", str(args.runs),
               "--seconds", str(args.seconds), "--files", str(args.files)]
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    if out.returncode:
        raise SystemExit("%s on %s failed (%d):\n%s" % (what, root, out.returncode, (out.stdout + out.stderr)[-2000:]))
    for line in reversed(out.stdout.splitlines()):
        if line.startswith("LONG_TIMING "):
            return json.loads(line[len("LONG_TIMING "):])["ms"]
        if line.startswith("{") and "ms_per_step" in line:
            return [json.loads(line)["ms_per_step"]]
    raise SystemExit("%s on %s printed no result" % (what, root))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_timing.txt"))
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--long-seconds", type=float, default=600.0)
    ap.add_argument("--windows", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: arm (d)")
    ap.add_argument("--worker", choices=("whole", "fileloop"), default=None)
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: at least 5 repeats")
    if args.worker:
        return worker(args)
    sys.path.insert(0, ROOT)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stat(ms):
        return "%9.2f  (%.2f .. %.2f, n = %d)" % (statistics.median(ms), min(ms), max(ms), len(ms))

    # ---- (d) first: the children need the GPU to themselves, before this process opens it
    cmp_rows = []
    if args.parent:
        parent = os.path.abspath(args.parent)
        for what, unit in (("whole", "ms per %.0f s file, whole-file plan, B = 1" % args.seconds),
                           ("fileloop", "ms per file, generate_wav over %d files of 4 s" % args.files),
                           ("bench", "ms per step, bench.py --gpus 1 --steps 30 --warmup 5")):
            got = {"parent": [], "this": []}
            for _ in range(args.rounds if what != "bench" else max(3, args.rounds)):
                for side, root in (("parent", parent), ("this", ROOT)):          # alternating
                    got[side] += child(root, what, args)
            cmp_rows.append((what, unit, got))
            print(what, {k: stat(v) for k, v in got.items()}, flush=True)

    import torch

    import __graft_entry__ as ge

    ge.build()
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    synth = importlib.import_module("prior-diffuse_amd.synth")
    pipeline = importlib.import_module("prior-diffuse_amd.pipeline")
    longplan = importlib.import_module("prior-diffuse_amd.longplan")
    nets = importlib.import_module("prior-diffuse_amd.nets")
    dev = "cuda:0"
    gs, ds = synth.make_state_dict("GCRN"), synth.make_state_dict("DiffUNet1")
    bank = nets.WeightBank()

    def size(ctx):
        return sum(t.numel() * t.element_size() for t in ctx.keep if torch.is_tensor(t))

    timed = lambda fn: _timed(torch, fn, args.runs)      # noqa: E731
    say("windowed passes over long recordings - %s, %d timed passes per figure after one untimed: median (min .. max)"
        % (torch.cuda.get_device_name(0), args.runs))
    L_ = int(args.seconds * 16000) // 160 * 160
    T = 1 + L_ // 160
    wav, x_T = synth.synthetic_waveforms(1, L_, seed=7)
    wav, x_T = wav.to(dev), x_T.to(dev)
    say()
    say("(a) one %.0f s file (T = %d frames), B = 1, GCRN prior, six fast steps, ms per file" % (args.seconds, T))
    whole = pipeline.SamplerPipeline(dev, "GCRN", gs, ds, 1, L_=L_, bank=bank, exclusive=False)
    ms = timed(lambda: whole.enhance(wav, x_T))
    whole.check()
    whole_ms, whole_bytes = statistics.median(ms), size(whole.ctx)
    say("    whole-file plan, launch by launch   %s" % stat(ms))
    ms = timed(lambda: whole.enhance(wav, x_T, graph=True))
    say("    whole-file plan, hipGraph replay    %s" % stat(ms))
    ref = whole.enhance(wav, x_T)[1]
    rows = []
    for W in args.windows:
        if T <= W:
            say("    window=%-5d                        the file fits the window: the whole-file plan" % W)
            continue
        long = pipeline.LongSampler(dev, "GCRN", gs, ds, 1, W, bank=bank)
        ms = timed(lambda: long.enhance(wav, x_T))
        long.check()
        med = statistics.median(ms)
        got = long.enhance(wav, x_T)[1]
        err = float((got.double() - ref.double()).norm() / ref.double().norm())
        ratio = longplan.recompute_ratio(W, *long.eps_field)
        nw, npw = len(long.eps_windows), len(long.prior_windows)
        say("    window=%-5d                        %s   %.2fx the whole-file plan" % (W, stat(ms), med / whole_ms))
        say("        %d eps-net windows x %d steps + %d prior windows; frames through the eps-net %d of %d = %.2fx "
            "(W / (W - %d - %d) = %.2fx for a file of many windows); rel-L2 against the whole-file spectrogram %.2e"
            % (nw, long.nsteps, npw, nw * W, T, nw * W / T, long.eps_field[0], long.eps_field[1], ratio, err))
        # the host side alone: the same loop with an empty plan range, then the copies by themselves
        stream = torch.cuda.current_stream().cuda_stream
        win = long.win

        def copies():
            for _ in range(long.nsteps):
                for a, lo, hi in long.eps_windows:
                    long._gather(long.x[0], win.audio, a, stream)
                    long._gather(long.init, win.eps.x_init, a, stream)
                    win.plan.run_range(0, 0, stream)
                    long._scatter(win.audio, long.x[1], a, lo, hi, stream)

        cms = timed(copies)
        moved = long.nsteps * sum(2 * (2 * 2 * W * 161 * 4) + 2 * (2 * (hi - lo) * 161 * 4) for _, lo, hi in long.eps_windows)
        say("        gathers, scatters and the empty run_range of all %d window steps alone: %s ms, %.1f us per window step of 3 "
            "launches + 1 call, %.0f GB/s over the bytes read and written" % (nw * long.nsteps, stat(cms), 1e3 * statistics.median(cms)
                                                                              / (nw * long.nsteps), moved / statistics.median(cms) / 1e6))
        rows.append((W, long.activation_bytes()))
        del long, win, got
    say()
    say("(b) activation bytes (per-plan device memory without the weights)")
    say("    whole-file plan, T = %-6d     %8.1f MiB  (%.1f KiB per frame)" % (T, whole_bytes / 2 ** 20, whole_bytes / T / 1024))
    for W, (win_b, side_b) in rows:
        say("    window=%-5d                   %8.1f MiB window plan + %.1f MiB whole-file side (%.1f KiB per frame)"
            % (W, win_b / 2 ** 20, side_b / 2 ** 20, side_b / T / 1024))
    per_frame = whole_bytes / T
    del whole, ref
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    say()
    say("(c) free device memory %.1f GiB of %.1f GiB (the allocator's report): a whole-file plan of %.0f KiB per frame records at most "
        "%d frames = %.1f minutes of signal, by arithmetic (nothing was allocated to find out)"
        % (free / 2 ** 30, total / 2 ** 30, per_frame / 1024, free // per_frame, free // per_frame / 6000.0))
    W = args.windows[0]
    L2 = int(args.long_seconds * 16000) // 160 * 160
    wav, x_T = synth.synthetic_waveforms(1, L2, seed=8)
    wav, x_T = wav.to(dev), x_T.to(dev)
    long = pipeline.LongSampler(dev, "GCRN", gs, ds, 1, W, bank=bank)
    ms = timed(lambda: long.enhance(wav, x_T))
    long.check()
    say("    a %.0f s recording (T = %d) through window=%d, ms per file: %s = %.2f ms per second of signal; "
        "window plan %.1f MiB + whole-file side %.1f MiB"
        % (args.long_seconds, 1 + L2 // 160, W, stat(ms), statistics.median(ms) / args.long_seconds,
           long.activation_bytes()[0] / 2 ** 20, long.activation_bytes()[1] / 2 ** 20))
    if cmp_rows:
        say()
        say("(d) this commit against its parent, child processes alternating parent / this commit in one session")
        for what, unit, got in cmp_rows:
            p, t = got["parent"], got["this"]
            inside = min(p) <= statistics.median(t) <= max(p)
            say("    %-9s parent %s   this %s   %s; this commit's median %s the parent's min .. max"
                % (what, stat(p), stat(t), unit, "inside" if inside else "OUTSIDE"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
