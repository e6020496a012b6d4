"""Diagnostic: per-launch hipEvent timings + algorithmic TFLOP/s of the GCRN prior at B=32, T=401.
--two-launches: GcrnPlan.fuse_phases off (every decoder stage as its two phase launches).  With it on, a fused pair's time is
printed on its even-bin row (with the GFLOP of both phases) and the odd-bin row shows '-'.
--tiled-proj: GcrnPlan.flat_proj off (the LSTM input projections, ops 5 and 6, in the tiled form of the other GEMM convolutions)."""
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
nets = importlib.import_module("prior-diffuse_amd.nets")
synth = importlib.import_module("prior-diffuse_amd.synth")
L = importlib.import_module("prior-diffuse_amd._lib")

B, T = int(os.environ.get("B", 32)), int(os.environ.get("T", 401))
nets.GcrnPlan.fuse_phases = "--two-launches" not in sys.argv[1:]
nets.GcrnPlan.flat_proj = "--tiled-proj" not in sys.argv[1:]
net = nets.GcrnPlan(nets.Ctx("cuda:0"), synth.make_state_dict("GCRN"), B, T)
net.build()
net.finish()
net.x.copy_(torch.randn(B, 2, T, 161))
n = len(net.descs)
runs = [net.plan.time_ops(0, n) for _ in range(5)][1:]
med = [statistics.median(r[i] for r in runs) * 1e3 for i in range(n)]
print("flat_proj %s" % nets.GcrnPlan.flat_proj)
print("fuse_phases %s: total %.1f us over %d ops, %d launches" % (nets.GcrnPlan.fuse_phases, sum(med), n, n - sum(
    1 for d, _ in net.descs if isinstance(d, L.GconvDesc) and d.korder == 5 and d.p1mask and not d.w2)))
print("%4s %-5s %4s %5s %5s %5s %6s %6s %9s %8s %7s" % ("op", "kind", "epi", "taps", "cin", "cout", "Tout", "Fout", "GFLOP", "us", "TF/s"))
def gflop(d):
    accs = 1 if d.epi == L.EPI_LINEAR else 2
    return 2.0 * d.B * d.Tout * d.Fout * accs * d.ntaps * max(d.in0.C + d.in1.C, 1) * d.Cout / 1e9


paired = False      # this operator ran inside the previous one's launch
for i, (d, tag) in enumerate(net.descs):
    if isinstance(d, L.GconvDesc):
        row = "%4d %-5s %4d %5d %5d %5d %6d %6d" % (i, "gconv", d.epi, d.ntaps, d.in0.C + d.in1.C, d.Cout, d.Tout, d.Fout)
        if paired:
            print("%s %9s %8s %7s" % (row, "-", "-", "-"))
            paired = False
            continue
        paired = bool(d.korder == 5 and d.p1mask and not d.w2)
        g, us = gflop(d), med[i]
        if paired:
            g, us = g + gflop(net.descs[i + 1][0]), us + med[i + 1]      # the event gap behind the launch belongs to it
        print("%s %9.2f %8.1f %7.1f" % (row, g, us, g / us * 1e3))
    else:
        print("%4d %-5s %61.1f" % (i, type(d).__name__[:5], med[i]))
