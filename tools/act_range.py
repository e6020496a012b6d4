"""Where the tensors the f16x2 kernels multiply sit in the fp16 window of include/pdse.h (PDSE_F16_ACT_EXP), for the nominal inputs
of the bench: the device report of an audited pass (``SamplerPipeline(audit=True).range_report()``, csrc/range.hip) - per marked
range and tensor the element count, the largest binade, the share of elements under the full-precision edge and the verdict.

    python tools/act_range.py [--prior GCRN] [-B 2] [-L 32000]
"""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--prior", default="GCRN")
    ap.add_argument("-B", type=int, default=2)
    ap.add_argument("-L", type=int, default=32000)
    a = ap.parse_args()
    ge.build()
    synth = importlib.import_module("prior-diffuse_amd.synth")
    Pk = importlib.import_module("prior-diffuse_amd.packing")
    pipeline = importlib.import_module("prior-diffuse_amd.pipeline")
    wav, x_T = synth.synthetic_waveforms(a.B, a.L, seed=1234)
    pipe = pipeline.SamplerPipeline("cuda:0", a.prior, synth.make_state_dict(a.prior), synth.make_state_dict("DiffUNet1"), a.B, L_=a.L,
                                    audit=True)
    pipe.enhance(wav.cuda(), x_T.cuda())
    pipe.check()
    rep = pipe.range_report()
    print("window: fp32-equivalent for %.4g <= |x|, hi leaves the fp16 range at %.5g" % (2.0 ** (-2 - Pk.F16_ACT_EXP), 65504.0 / 2 ** Pk.F16_ACT_EXP))
    print(rep)
    print("ok" if rep.ok else "NOT ok: worst %r" % rep.worst())


if __name__ == "__main__":
    main()
