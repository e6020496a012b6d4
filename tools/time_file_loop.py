"""Time the B = 1 file loop, ``ComplexDDPMTrainer.generate_wav``, on directories of wav files at a given sample rate: what a
file costs from the wav read (decode, mono mix, conversion to 16 kHz) to the written result.  16 synthetic 4 s files per rate,
one untimed run (weights, plan, graph capture), then three timed runs; prints the median ms per file with the lowest and the
highest run.  Only the public interface is used, so the same script times any checkout of the project:

    python tools/time_file_loop.py [--rates 16000 44100 48000] [--root OTHER_CHECKOUT] [--files 16] [--seconds 4] [--runs 3]
                                   [--format s16|s24|f32|f64|ulaw] [--channels N] [--wav-out pcm16|source] [--per-channel]
                                   [--distinct-channels]

--format other than s16, or --channels above 1, writes the files with a RIFF writer of this script's own and times
``generate_wav`` of a trainer built with ``wav_formats="all"`` (s16 with more channels goes through the same trainer, so the
three formats are compared on one loop); the default - 16-bit mono through the default trainer - needs nothing a checkout
before ``wav_formats`` lacks.

--wav-out source times the same loop of a trainer built with ``wav_out="source"``: every file is written at its source's rate,
length, channel count and encoding, converted and encoded on the device (``wavdev.encode``), instead of 16 kHz, 16-bit, mono.
The default passes nothing, so a checkout before ``wav_out`` is timed by the same command (profiles/wav_out_timing.txt).

--per-channel times the loop of a trainer built with ``channels="each"``: every channel of a file is enhanced on its own (one exact
ragged pass of B = channels per file) and the file is written with that many different channels (``wavdev.encode_channels``).  The
files' channels then differ - channel c is the signal of seed 100 + i + 1000 c - so that nothing can be shared between them; without
the flag the files are written as before, or with --distinct-channels as --per-channel writes them, so that both loops read the
same files (profiles/wav_channels_timing.txt).

Lines of several invocations (say, this commit and its parent, alternating) are collected in profiles/wav_frontend_timing.txt
and profiles/wav_formats_timing.txt.
"""
import argparse
import importlib
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


FORMATS = {"s16": (1, 2), "s24": (1, 3), "f32": (3, 4), "f64": (3, 8), "ulaw": (7, 1)}      # name -> (format tag, bytes per sample)


def write_file(path, x, rate, fmt, channels, np):
    """x: mono float samples in [-1, 1); every channel holds them (the mix is then x again up to the encoding's rounding).
    x [channels, n]: the channels' own samples."""
    tag, width = FORMATS[fmt]
    repeat = channels
    if np.ndim(x) == 2:
        x, repeat = np.asarray(x).T.reshape(-1), 1            # interleaved here; nothing to repeat
    x = np.clip(np.asarray(x, dtype=np.float64), -1.0, 1.0 - 2.0 ** -15)
    if fmt == "s16":
        data = np.round(x * 32768.0).astype("<i2")
    elif fmt == "s24":
        data = np.round(x * 8388608.0).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]
    elif fmt == "ulaw":         # G.711 compression of the 16-bit value: bias 0x84, segment = position of the leading one
        v = np.round(x * 32768.0).astype(np.int32)
        mag = np.minimum(np.abs(v), 32635) + 0x84
        seg = np.floor(np.log2(mag)).astype(np.int32) - 7
        data = (~(np.where(v < 0, 0x80, 0) | (seg << 4) | ((mag >> (seg + 3)) & 15)) & 0xFF).astype(np.uint8)
    else:
        data = x.astype("<f4" if fmt == "f32" else "<f8")
    data = np.repeat(data.reshape(x.size, -1), repeat, axis=0).tobytes()
    head = struct.pack("<HHIIHH", tag, channels, rate, rate * channels * width, channels * width, 8 * width)
    body = b"WAVEfmt " + struct.pack("<I", 16) + head + b"data" + struct.pack("<I", len(data)) + data + b"\0" * (len(data) & 1)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", type=int, nargs="+", default=[16000, 44100, 48000])
    ap.add_argument("--root", default=HERE, help="the checkout to time (default: the one this script lies in)")
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--label", default=None)
    ap.add_argument("--format", choices=sorted(FORMATS), default="s16")
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--wav-out", choices=("pcm16", "source"), default="pcm16")
    ap.add_argument("--per-channel", action="store_true")
    ap.add_argument("--distinct-channels", action="store_true", help="the files --per-channel writes, for the loop without it")
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
        all_wav = args.format != "s16" or args.channels > 1 or args.per_channel
        tr = trainer.ComplexDDPMTrainer(
            ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav=os.path.join(work, "out")),
            ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
            device="cuda:0", prior_state_dict=synth.make_state_dict("GCRN"), ddpm_state_dict=synth.make_state_dict("DiffUNet1"),
            **({"wav_formats": "all"} if all_wav else {}), **({"wav_out": "source"} if args.wav_out == "source" else {}),
            **({"channels": "each"} if args.per_channel else {}))
        for rate in args.rates:
            src = os.path.join(work, "in_%d" % rate)
            os.makedirs(src)
            n = int(round(args.seconds * rate))
            for i in range(args.files):
                if args.per_channel or args.distinct_channels:
                    x = np.stack([np.asarray(synth.speechlike(1, n, 100 + i + 1000 * c)[0]) for c in range(args.channels)])
                    write_file(os.path.join(src, "f%02d.wav" % i), x, rate, args.format, args.channels, np)
                elif all_wav:
                    write_file(os.path.join(src, "f%02d.wav" % i), synth.speechlike(1, n, 100 + i)[0], rate, args.format, args.channels, np)
                else:
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
            res = {"label": label, "rate": rate, "format": args.format, "channels": args.channels,
                   "loop": "wav_formats=all" if all_wav else "default", "wav_out": args.wav_out,
                   "channel_mode": "each" if args.per_channel else "mix", "files": args.files, "seconds_per_file": args.seconds,
                   "ms_per_file_median": round(statistics.median(ms), 3), "ms_per_file_min": round(min(ms), 3),
                   "ms_per_file_max": round(max(ms), 3), "runs": args.runs}
            print("%-10s %-4s x%d %6d Hz -> %-6s %-4s: %8.3f ms per file (%.3f .. %.3f over %d runs of %d files of %.1f s)" % (
                label, args.format, args.channels, rate, args.wav_out, res["channel_mode"], res["ms_per_file_median"], res["ms_per_file_min"], res["ms_per_file_max"], args.runs, args.files,
                args.seconds), flush=True)
            print("RESULT " + json.dumps(res), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
