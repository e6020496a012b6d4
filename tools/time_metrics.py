"""Time metrics.quality on the device (hipEvents, warm-up, median of 30) at B=32 x 4 s and B=1 x 4 s, next to the sequential
SamplerPipeline.enhance pass of the same batch in the same process, and write the device section of
profiles/metrics_timing.txt.  Sections of that file that come from elsewhere (the reference's CPU cost, per-kernel shares)
are kept: only the paragraph that starts with DEVICE_HEAD is replaced.

    python tools/time_metrics.py [--out profiles/metrics_timing.txt]
"""
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup=5, reps=30):
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


DEVICE_HEAD = "metrics.quality (SSNR + LLR + WSS + fwSNRseg), hipEvent times in ms"


def merge(old, device_text):
    """Replace the device paragraph of the file's text (or append one); every other paragraph stays."""
    paras = [p for p in old.split("\n\n") if p.strip() and not p.lstrip().startswith(DEVICE_HEAD)]
    return "\n\n".join([p.strip("\n") for p in paras] + [device_text.strip("\n")]) + "\n"


def main():
    import numpy as np
    import torch

    import __graft_entry__ as ge

    ge.build()
    synth = importlib.import_module("prior-diffuse_amd.synth")
    metrics = importlib.import_module("prior-diffuse_amd.metrics")
    pipeline = importlib.import_module("prior-diffuse_amd.pipeline")
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "metrics_timing.txt")
    B, L_ = 32, 64000
    clean = synth.speechlike(B, L_, 77)
    noise = np.random.RandomState(78).standard_normal(clean.shape).astype(np.float32)
    c, p = torch.from_numpy(clean).cuda(), torch.from_numpy(clean + 0.05 * noise).cuda()
    lines = [DEVICE_HEAD + ": median (min .. max) of 30 after 5 warm-up calls"]
    q32 = timed(lambda: metrics.quality(c, p))
    lines.append("quality  B=32 x 4 s : %.3f (%.3f .. %.3f)" % q32)
    lines.append("quality  B=1  x 4 s : %.3f (%.3f .. %.3f)" % timed(lambda: metrics.quality(c[:1], p[:1])))
    c10 = torch.from_numpy(synth.speechlike(1, 160000, 79)).cuda()
    lines.append("quality  B=1  x 10 s: %.3f (%.3f .. %.3f)" % timed(lambda: metrics.quality(c10, c10 * 0.9)))
    gs, ds = synth.make_state_dict("GCRN"), synth.make_state_dict("DiffUNet1")
    wav, x_T = synth.synthetic_waveforms(B, L_, seed=1234)
    pipe = pipeline.SamplerPipeline("cuda:0", "GCRN", gs, ds, B, L_=L_, fast_sampling=True)
    wav, x_T = wav.cuda(), x_T.cuda()
    e32 = timed(lambda: pipe.enhance(wav, x_T), warmup=3, reps=20)
    lines.append("enhance  B=32 x 4 s : %.3f (%.3f .. %.3f)   sequential SamplerPipeline.enhance, GCRN prior, fast sampling" % e32)
    lines.append("scoring / enhancing at B=32: %.3f" % (q32[0] / e32[0]))
    text = "\n".join(lines) + "\n"
    print(text)
    old = open(out).read() if os.path.exists(out) else ""
    with open(out, "w") as f:
        f.write(merge(old, text))


if __name__ == "__main__":
    main()
