"""On the GPU box: time per launch of every compand mode (csrc/misc.hip) and of pdse_spec_frames_mode (csrc/valid.hip) at the
BASELINE geometry B = 32, T = 401, beside the sqrt modes and beside the copy rate of the project's elementwise kernel (EW_COPY of
the same tensor, timed in the same run).

    python tools/time_feat_type.py [--B 32] [--T 401] [--inner 20] [--runs 30] [--out profiles/feat_type_timing.txt]

Device events around ``--inner`` back-to-back launches, the median of ``--runs`` such groups (lowest .. highest) after 3 warm-up
groups; bytes = one read and one write of the [B,2,T,161] fp32 tensor for the compand launches (the scattered output: the same
bytes), one read of it and one write of [B,320,T] for the frame kernel."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("0 mag**0.5 (sqrt, compress)", "1 mag**2 (sqrt, decompress)", "2 mag (normal, compress)", "3 copy (normal / none, decompress)",
         "4 mag**0.3 (cubic, compress)", "5 mag**(10/3) (cubic, decompress)", "6 log(mag+1) (log_1x, compress)",
         "7 exp(mag)-1 (log_1x, decompress)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=401)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feat_type_timing.txt"))
    a = ap.parse_args()
    import __graft_entry__ as ge

    ge.build()
    L = importlib.import_module("prior-diffuse_amd._lib")
    ops = importlib.import_module("prior-diffuse_amd.ops")
    dev = torch.device("cuda:0")
    B, T, F = a.B, a.T, 161
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(B, 2, T, F, generator=g) * 1.5).to(dev)
    out = torch.empty_like(x)
    rows = torch.zeros(B, T, 2 * 168, device=dev)
    frames = torch.empty(B, 320, T, device=dev)
    basis, _ = ops.frame_tables(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn):
        ms = []
        for k in range(3 + a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            if k >= 3:
                ms.append(e0.elapsed_time(e1) / a.inner)
        return float(np.median(ms)), min(ms), max(ms)

    def compand(mode, scattered):
        d = L.CompandDesc()
        d.in_, d.plane, d.B, d.mode = x.data_ptr(), T * F, B, mode
        if scattered:
            d.out, d.out_sb, d.out_sc, d.out_st, d.F = rows.data_ptr(), T * 336, 168, 336, F
        else:
            d.out = out.data_ptr()
        return lambda: L.launch(d, stream, device=dev)

    ew = L.EwDesc()
    ew.a, ew.out, ew.n, ew.op = x.data_ptr(), out.data_ptr(), x.numel(), L.EW_COPY
    nbytes = 2 * x.numel() * 4
    copy = timed(lambda: L.launch(ew, stream, device=dev))
    rate = nbytes / copy[0] / 1e6
    lines = ["compand modes and pdse_spec_frames_mode, B = %d, T = %d (%.1f MB read + written per compand launch), ms per launch:" % (B, T, nbytes / 1e6),
             "median of %d groups of %d launches [lowest .. highest], GB/s, share of the EW_COPY rate measured in this run" % (a.runs, a.inner),
             "  %-52s %.4f [%.4f .. %.4f] %7.0f GB/s   1.00" % (("EW_COPY of the same tensor (csrc/misc.hip ew_kernel)",) + copy + (rate,))]
    for mode, name in enumerate(NAMES):
        for scattered in (False, True):
            if scattered and mode not in (L.COMPAND_SQUARE, L.COMPAND_COPY, L.COMPAND_POW103, L.COMPAND_EXPM1):
                continue
            r = timed(compand(mode, scattered))
            gbs = nbytes / r[0] / 1e6
            lines.append("  %-52s %.4f [%.4f .. %.4f] %7.0f GB/s   %.2f" % (("compand " + name + (", F > 0 rows" if scattered else "")[:52],) + r + (gbs, gbs / rate)))
    fbytes = (x.numel() + frames.numel()) * 4
    for mode in (L.COMPAND_SQUARE, L.COMPAND_COPY, L.COMPAND_POW103, L.COMPAND_EXPM1):
        r = timed(lambda: L.spec_frames_mode(x.data_ptr(), basis.data_ptr(), frames.data_ptr(), B, T, F, mode, stream, device=dev))
        lines.append("  %-52s %.4f [%.4f .. %.4f] %7.0f GB/s   (double sums: not a memory-rate kernel)" % (
            ("spec_frames_mode, mode %d" % mode,) + r + (fbytes / r[0] / 1e6,)))
    print("\n".join(lines))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
