"""Time metrics.quality(stoi=True) next to metrics.quality() on one B = 32 x 4 s batch in one process (hipEvents, warm-up,
median of 30) and write profiles/stoi_timing.txt.  Run it under a time limit of its own:

    timeout -k 10 300 python tools/time_stoi.py [--out profiles/stoi_timing.txt]
"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_metrics import timed  # noqa: E402


def main():
    import numpy as np
    import torch

    import __graft_entry__ as ge

    ge.build()
    synth = importlib.import_module("prior-diffuse_amd.synth")
    metrics = importlib.import_module("prior-diffuse_amd.metrics")
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "stoi_timing.txt")
    B, L_ = 32, 64000
    clean = synth.speechlike(B, L_, 77)
    noise = np.random.RandomState(78).standard_normal(clean.shape).astype(np.float32)
    c, p = torch.from_numpy(clean).cuda(), torch.from_numpy(clean + 0.05 * noise).cuda()
    q = metrics.quality(c, p, stoi=True)
    lines = ["metrics.quality with and without STOI / ESTOI on one MI355X, hipEvent times in ms: median (min .. max) of 30 after 5 "
             "warm-up calls, same process, same batch (every call allocates its own outputs and workspace)"]
    plain = timed(lambda: metrics.quality(c, p))
    both = timed(lambda: metrics.quality(c, p, stoi=True))
    one = timed(lambda: metrics.quality(c[:1], p[:1], stoi=True))
    lines.append("quality()           B=32 x 4 s : %.3f (%.3f .. %.3f)" % plain)
    lines.append("quality(stoi=True)  B=32 x 4 s : %.3f (%.3f .. %.3f)" % both)
    lines.append("the four STOI launches, by difference of the medians: %.3f" % (both[0] - plain[0]))
    lines.append("quality(stoi=True)  B=1  x 4 s : %.3f (%.3f .. %.3f)" % one)
    lines.append("mean STOI %.4f, mean ESTOI %.4f of the batch" % (float(q["stoi"].mean()), float(q["estoi"].mean())))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
