"""Case tables and the descriptor builder shared by tests/test_gconv_refs_host.py (CPU tensors, replayed on tests/emu.py)
and tests/test_gpu_gconv_ops.py (the HIP kernels), so that the two files cannot drift apart.

A case is a dict over DEFAULTS.  ``build`` turns it into one pdse_gconv_desc through PlanBase.gconv - the same packers and
the same routing the networks use - on tensors laid out for the two structural checks of the GPU file:
  * every input sits inside a larger allocation whose margins (one frame and one bin on each side) hold NaN: a gather
    that reads beyond [0,Tin) x [0,Fin) instead of taking zero poisons the output;
  * the output is a NaN-filled buffer with a margin on either side of the addressed box and gaps inside it (every stride
    larger than dense): after the launch exactly the addressed elements are finite, every other one is still the NaN
    it was, bit for bit.
Inputs: seeded N(0,1) activations, N(0, 1/K) weights, PReLU slope 0.25, post_scale from U(0.5, 1.5)."""
import math
import zlib

import numpy as np
import torch

from conftest import pkg, rel_l2
from helpers import gconv_refs as R

NONE, PRELU, ELU, SIGMOID = R.ACT_NONE, R.ACT_PRELU, R.ACT_ELU, R.ACT_SIGMOID
LIN, GLU = R.EPI_LINEAR, R.EPI_GLU
MARGIN = 8                      # floats in front of and behind the output box (keeps the base 16-byte aligned)
SLOPE = 0.25

# ---- tap tables -----------------------------------------------------------------------------------------------------
TAPS = {
    "1x1": [(0, 0)],
    "c23": [(dt, df) for dt in (-1, 0) for df in (-1, 0, 1)],                  # causal (2,3), same padding over the bins
    "s2": [(dt, df) for dt in (-1, 0) for df in (0, 1, 2)],                    # the same kernel at bin stride 2 (sf_in = 2)
    "tp0": [(-kt, -(kf // 2)) for kt in (0, 1) for kf in (0, 2)],              # (2,3) stride-(1,2) transposed conv, even bins
    "tp1": [(-kt, 0) for kt in (0, 1)],                                        # ... odd bins
    "r3": [(0, -1), (0, 0), (0, 1)],                                           # DB-AIAT (1,3) convolutions
    "e3": [(0, 0), (0, 1), (0, 2)],                                            # GCRN encoder (1,3) at bin stride 2
    "d2": [(0, 0), (0, -1)],                                                   # GCRN decoder (1,3) stride-(1,2), even bins
    "tcm5": [(2 * (k - 2), 0) for k in range(5)],                              # TCM dilated Conv1d, dilation 2
    "pad5": [(-2, 0), (-1, -1), (-1, 0), (-1, 1), (0, 0)],                     # frames -2, -1 (the pad row) and 0
    "bins5": [(0, k) for k in range(5)],                                       # Linear over 5 / 8 bins (cin1)
    "bins8": [(0, k) for k in range(8)],
    "stft6": [(0, k) for k in range(6)],                                       # frames of 6 samples, hop 3 (cin1, sf_in = 3)
    "k34": [(dt, df) for dt in (-1, 0, 1) for df in (-2, -1, 0, 1)],           # 12 taps leaving the tensor on all four sides
}

DEFAULTS = dict(B=1, C0=2, C1=0, Cout=32, taps="1x1", sf_in=1, Tout=3, Fout=11, Fin=None, epi=LIN, act=NONE, post=False,
                bias="shared", resid=False, layout="nchw", out_off=0, padrow=False, xf=0, act1=NONE, cin1=False, blk=False,
                wscale=1.0)

P1, P33, P127, P129 = dict(Tout=1, Fout=1), dict(Tout=3, Fout=11), dict(Tout=1, Fout=127), dict(Tout=3, Fout=43)
G1, G255, G257 = dict(Tout=1, Fout=1), dict(Tout=5, Fout=51), dict(Tout=1, Fout=257)
S2 = dict(taps="s2", sf_in=2, Fin=9, Fout=4)


def _c(name, **kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, id=name, **kw)


# ---- generic kernel (korder 0: csrc/gconv.hip), PlanBase.force_generic ------------------------------------------------
# store paths of gconv_epilogue_impl: "tile" = full 32-channel tile with a plain channel stride, "elem" = the element-wise
# path (partial tile, or out_cr != 1 without the blocked form), "c16" = channels innermost 16-byte stores, "b16" = blocked
GENERIC = [
    # channels (pair loop, its unroll-4 tail, second-source base) x Cout (partial tiles, MT 1 / 2 / 4, dead tiles) x positions
    _c("c2_lin_cout33_p129", C0=2, Cout=33, taps="c23", **P129),                        # MT 2: tile + elem
    _c("c6_glu_cout31_p33", C0=6, Cout=31, taps="c23", epi=GLU, **P33),                 # MT 1: elem
    _c("c34_lin_cout1_p127", C0=34, Cout=1, **P127),
    _c("c34_glu_cout33_p33", C0=34, Cout=33, epi=GLU, **P33),
    _c("c2_lin_cout1_p1", C0=2, Cout=1, **P1),
    _c("c2c4_lin_cout96_p129", C0=2, C1=4, Cout=96, taps="c23", **P129),                # MT 2, half-empty last z-slice
    _c("c2c4_glu_cout96_tp0_p33", C0=2, C1=4, Cout=96, taps="tp0", epi=GLU, **P33),
    _c("c6_lin_cout128_p127", C0=6, Cout=128, **P127),                                  # MT 4
    _c("c6_lin_cout160_p33", C0=6, Cout=160, taps="tp1", **P33),                        # MT 4, three dead tiles in z = 1
    _c("c2c4_glu_cout128_p1", C0=2, C1=4, Cout=128, epi=GLU, **P1),
    _c("c6_glu_cout160_p129", C0=6, Cout=160, epi=GLU, **P129),
    _c("c6_lin_s2_cout33", C0=6, Cout=33, Tout=5, **S2),
    _c("c2c4_glu_s2_cout31", C0=2, C1=4, Cout=31, epi=GLU, Tout=5, **S2),
    _c("c6_lin_tp0_cout33_p129", C0=6, Cout=33, taps="tp0", **P129),
    _c("c6_lin_tp1_cout33_p129", C0=6, Cout=33, taps="tp1", **P129),
    # cin1
    _c("cin1_bins5_cout33", C0=1, cin1=True, taps="bins5", Fin=5, Tout=33, Fout=1, Cout=33),
    _c("cin1_bins8_cout33", C0=1, cin1=True, taps="bins8", Fin=8, Tout=33, Fout=1, Cout=33, act=SIGMOID),
    _c("cin1_stft_cout10_cr5", C0=1, cin1=True, taps="stft6", sf_in=3, Fin=3 * 36 + 6, Tout=1, Fout=37, Cout=10, layout="stft",
       bias="none", B=2),
    # pad row: frame -1 reads the row, frames <= -2 and out-of-range bins read zero
    _c("padrow_c2c4_b2", B=2, C0=2, C1=4, Cout=33, taps="pad5", padrow=True, **P33),
    _c("padrow_c2c4_glu", B=2, C0=2, C1=4, Cout=32, taps="pad5", padrow=True, epi=GLU, **P33),
    # load transform (non-zero shifts: transforming the zero padding would show)
    _c("xf1_lin_c6", C0=6, Cout=33, taps="c23", xf=1, **P33),
    _c("xf2_glu_c6", C0=6, Cout=33, taps="tcm5", xf=2, epi=GLU, Tout=33, Fout=1),
    # ELU on in1 only
    _c("elu_in1_lin", C0=2, C1=4, Cout=33, taps="c23", act1=ELU, **P33),
    _c("elu_in1_glu", C0=2, C1=4, Cout=32, taps="d2", act1=ELU, epi=GLU, **P33),
    # epilogue
    _c("bias_none_lin", C0=6, Cout=33, bias="none", **P33),
    _c("bias_item_lin", B=2, C0=6, Cout=33, bias="item", **P33),
    _c("bias_item_glu_post", B=2, C0=6, Cout=33, bias="item", post=True, epi=GLU, **P33),
    _c("post_lin_prelu", C0=6, Cout=33, post=True, act=PRELU, **P33),
    _c("lin_elu", C0=6, Cout=64, act=ELU, **P33),
    _c("lin_sigmoid", C0=6, Cout=33, act=SIGMOID, **P33),
    _c("glu_prelu", C0=6, Cout=64, epi=GLU, act=PRELU, **P33),
    _c("glu_elu_post", C0=6, Cout=33, epi=GLU, act=ELU, post=True, **P33),
    _c("glu_sigmoid", C0=6, Cout=32, epi=GLU, act=SIGMOID, **P33),
    _c("resid_lin", C0=6, Cout=33, resid=True, **P33),
    _c("resid_glu", C0=6, Cout=64, resid=True, epi=GLU, post=True, **P33),
    _c("out_off_lin", C0=6, Cout=33, out_off=3, **P33),
    _c("clast_aligned_lin", C0=6, Cout=64, layout="clast", act=PRELU, post=True, **P33),            # c16
    _c("clast_off1_lin", C0=6, Cout=64, layout="clast", out_off=1, act=PRELU, post=True, **P33),    # its fallback
    _c("clast_aligned_cout33", C0=6, Cout=33, layout="clast", **P33),                               # c16 + elem
    _c("clast_resid", C0=6, Cout=32, layout="clast", resid=True, **P33),
    _c("blk8_cout48_lin", C0=6, Cout=48, layout="blk8", act=ELU, post=True, **P33),                 # b16 + elem
    _c("blk8_cout48_glu", C0=6, Cout=48, layout="blk8", epi=GLU, bias="item", B=2, **P33),
    _c("blk8_off1_cout32", C0=6, Cout=32, layout="blk8", out_off=1, **P33),                         # blocked fallback
]
for _x in GENERIC:
    _x.update(family="generic", korder=0)

# ---- pipelined kernel (korder 1: csrc/gconv2.hip) -------------------------------------------------------------------
# one entry per LINEAR / GLU row of packing.V2_CP / pdse_gconv2_launch: (epi, taps of the layer the row serves, two sources,
# xf_mode, CP, extra); each at a source width that fills its CP-pair chunks (Cout 33) and one that does not (Cout 32)
V2_ROWS = [
    ("lin_t1", LIN, "1x1", False, 0, 8, {}),
    ("lin_t1_xf1", LIN, "1x1", False, 1, 8, {}),
    ("lin_t1_two", LIN, "1x1", True, 0, 8, {}),
    ("lin_t4", LIN, "tp0", False, 0, 2, {}),
    ("lin_t3", LIN, "r3", False, 0, 4, {}),
    ("lin_t6", LIN, "c23", False, 0, 2, {}),
    ("glu_t1_two", GLU, "1x1", True, 0, 4, dict(act1=ELU)),
    ("glu_t2_two", GLU, "d2", True, 0, 2, dict(act1=ELU)),
    ("glu_t3", GLU, "e3", False, 0, 4, dict(sf_in=2, Fin=88, act=ELU, post=True)),
    ("glu_t5_xf2", GLU, "tcm5", False, 2, 4, dict(Tout=129, Fout=1)),
]
V2_WIDTHS = {8: (16, 18), 4: (8, 6), 2: (4, 6)}


def _k1_cases():
    out = []
    for name, epi, taps, two, xf, cp, extra in V2_ROWS:
        full, part = V2_WIDTHS[cp]
        for c, cout in ((full, 33), (part, 32)):
            kw = dict(P129, C0=c, C1=(full + part - c) if two else 0, Cout=cout, epi=epi, taps=taps, xf=xf)
            kw.update(extra)
            out.append(_c("%s_c%d_cout%d" % (name, c, cout), **kw))
    return out


K1 = _k1_cases()


def pick_mt(B, P, Cout, max_mt):
    """The rule in pick_mt's comment (csrc/gconv2.hip): a wave takes 2 (4) channel tiles only where that still leaves
    2048 waves - B * ceil(P / 32) * ceil(mtiles / MT) >= 2048."""
    tiles, mtiles, mt = B * ((P + 31) // 32), (Cout + 31) // 32, 1
    cand = 2
    while cand <= max_mt and cand <= mtiles:
        if tiles * ((mtiles + cand - 1) // cand) >= 2048:
            mt = cand
        cand *= 2
    return mt


def widening_shape(Cout, max_mt, want):
    """Smallest B * ceil(Tout * Fout / 32) (a power of two, as (B, Tout, Fout) with Fout = 256) at which pick_mt returns
    ``want`` for Cout channels."""
    tiles = 1
    while pick_mt(1, 32 * tiles, Cout, max_mt) != want:
        tiles *= 2
        assert tiles <= 1 << 14
    B = 4
    Tout = tiles * 32 // (B * 256)
    assert B * Tout * 256 == 32 * tiles
    return dict(B=B, Tout=Tout, Fout=256)


K1_WIDE = [      # (case, MT the launch must take, widest MT of the epilogue)
    (_c("wide_lin_mt4", C0=16, Cout=128, **widening_shape(128, 4, 4)), 4, 4),
    (_c("wide_lin_mt2", C0=16, Cout=128, **widening_shape(128, 4, 2)), 2, 4),
    (_c("wide_glu_mt2", C0=8, C1=6, Cout=128, epi=GLU, act1=ELU, **widening_shape(128, 2, 2)), 2, 2),
]
for _x in K1 + [w[0] for w in K1_WIDE]:
    _x.update(family="k1", korder=1)

# ---- GEMM-shaped kernel (korder 3 / 4 / 5: csrc/gconv4.hip), the same table for the three of them ----------------------
# K loop: chunks of G4_CH = 3 sixteen-channel blocks of one (source, tap) - 16, 32, 64 channels leave a partial chunk
GEMM = [
    _c("c16_t1_lin16_p1", C0=16, Cout=16, **G1),                                                   # MT 1, elem
    _c("c32_t2_lin48_p255", C0=32, Cout=48, taps="d2", **G255),                                    # MT 2: tile + elem
    _c("c48_t6_lin128_p257", C0=48, Cout=128, taps="c23", **G257),                                 # MT 4 (korder 3: large LDS)
    _c("c64_t12_lin160_p255", C0=64, Cout=160, taps="k34", **G255),                                # MT 4, three dead tiles
    _c("c16c48_t6_glu32_p257", C0=16, C1=48, Cout=32, taps="c23", epi=GLU, **G257),                # GLU MT 1
    _c("c48c16_t2_glu48_p255", C0=48, C1=16, Cout=48, taps="d2", epi=GLU, **G255),                 # GLU MT 2, partial tile
    _c("c64_t1_glu64_p257", C0=64, Cout=64, epi=GLU, **G257),                                      # GLU MT 2 (korder 3: large LDS)
    _c("c16_t12_glu64_p255", C0=16, Cout=64, taps="k34", epi=GLU, **G255),
    _c("c32_s2_lin16", C0=32, Cout=16, Tout=5, **S2),
    _c("c16c48_s2_glu48", C0=16, C1=48, Cout=48, epi=GLU, Tout=5, **S2),
    _c("elu_in1_c16c48_glu48", C0=16, C1=48, Cout=48, taps="d2", epi=GLU, act1=ELU, act=ELU, post=True, **G255),
    _c("elu_in1_c48c16_lin48", C0=48, C1=16, Cout=48, taps="c23", act1=ELU, **G255),
    _c("blk_c32_lin48", C0=32, Cout=48, taps="c23", blk=True, **G255),
    _c("blk_c16c48_glu32", C0=16, C1=48, Cout=32, taps="k34", blk=True, epi=GLU, **G257),
    _c("out_blk8_c16_lin32", C0=16, Cout=32, taps="d2", layout="blk8", **G255),                    # b16
    _c("out_blk8_c32_glu48", C0=32, Cout=48, taps="c23", layout="blk8", epi=GLU, act=ELU, post=True, **G257),   # b16 + elem
    _c("item_bias_post_prelu_lin128", B=2, C0=16, Cout=128, bias="item", post=True, act=PRELU, **G255),
    _c("resid_glu32", B=2, C0=32, Cout=32, taps="d2", epi=GLU, resid=True, **G255),
    _c("clast_lin128", C0=16, Cout=128, layout="clast", **G255),                                   # c16 (the LSTM gate buffer)
]
for _x in GEMM:
    _x.update(family="gemm")
GEMM_WSCALE = [_c("k5_wscale_2e%d" % e, C0=48, Cout=48, taps="c23", wscale=2.0 ** e, **G255) for e in (-10, 6)]
for _x in GEMM_WSCALE:
    _x.update(family="gemm")
CHAIN = (_c("chain_a", B=2, C0=32, Cout=48, taps="c23", layout="blk8pad", act=ELU, post=True, Tout=5, Fout=51),
         _c("chain_b", B=2, C0=48, Cout=32, taps="k34", blk=True, epi=GLU, Tout=5, Fout=51))
for _x in CHAIN:
    _x.update(family="gemm")

PLANES_OF = {3: 3, 4: 1, 5: 2}


def by_id(cases):
    return [c["id"] for c in cases]


# ---- builder ----------------------------------------------------------------------------------------------------------
def _layout(case):
    """(out_strides (sb, sc_hi, sc_lo, st, sf), out_cr, out_off) - every stride leaves a gap."""
    Co, To, Fo, off = case["Cout"], case["Tout"], case["Fout"], case["out_off"]
    lay = case["layout"]
    if lay == "nchw":
        st = Fo + 1
        sc = To * st + 3
        return (Co * sc + 5, sc, 0, st, 1), 1, off
    if lay == "clast":          # channels innermost; 16-byte stores want every stride in multiples of 4 floats
        sf = 4 * ((Co + 3) // 4) + 4
        st = Fo * sf + 4
        return (To * st + 8, 1, 0, st, sf), 1, off
    if lay == "blk8":           # [B][C/8][T][F][8]
        st = 8 * Fo + 8
        sc = To * st + 8
        return (((Co + 7) // 8) * sc + 8, sc, 1, st, 8), 8, off
    if lay == "blk8pad":        # the same with a frame and a bin of margin on each side (read back by a blk = 8 source)
        st = 8 * (Fo + 2)
        sc = (To + 2) * st
        return (((Co + 7) // 8) * sc, sc, 1, st, 8), 8, st + 8
    if lay == "stft":           # channel index split over (re / im, bin): out_cr bins innermost
        cr = Co // 2
        sf = cr + 1
        st = Fo * sf + 1
        sc = To * st + 2
        return (2 * sc + 3, sc, 1, st, sf), cr, off
    raise KeyError(lay)


class Built:
    pass


def seed_of(case):
    return zlib.crc32(case["id"].encode())


def build(case, device, korder=None, src=None, src_ref=None):
    """Record the case as one descriptor on ``device``.  korder: 3 / 4 / 5 for the gemm family.  src: (buffer, element
    offset, (sb, sc, st, sf)) of a blocked tensor an earlier launch wrote (in0 then comes from there, src_ref being its
    reference value); returns a Built with desc, buf (the whole output allocation), index (flat positions of the
    addressed elements [B, Cout, Tout, Fout]) and ref(dtype) -> the reference evaluated in that dtype."""
    nets, L = pkg("nets"), pkg("_lib")
    g = torch.Generator().manual_seed(seed_of(case))
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)                    # noqa: E731
    uni = lambda *s: 0.5 + torch.rand(*s, generator=g, dtype=torch.float32)                 # noqa: E731
    c = case
    B, C0, C1, Co, To, Fo = c["B"], c["C0"], c["C1"], c["Cout"], c["Tout"], c["Fout"]
    Cin, taps, epi = C0 + C1, TAPS[c["taps"]], c["epi"]
    Tin, Fin = To, (c["Fin"] if c["Fin"] else Fo)
    pb = nets.PlanBase(nets.Ctx(device), plan=None)
    fam = c["family"]
    if fam == "generic":
        pb.force_generic = True
    elif fam == "gemm":
        pb.gemm_planes = PLANES_OF[korder]
    dev = lambda t: t.contiguous().to(device)                                               # noqa: E731
    keep = []

    def source(C_, a, data):
        """data [B, C_, Tin, Fin] inside a NaN allocation with a frame and a bin of margin on each side."""
        if c["blk"]:
            big = torch.full((B, C_ // 8, Tin + 2, Fin + 2, 8), math.nan)
            big[:, :, 1:-1, 1:-1] = data.view(B, C_ // 8, 8, Tin, Fin).permute(0, 1, 3, 4, 2)
            st = (Fin + 2) * 8
            strides, off, blk = (C_ // 8 * (Tin + 2) * st, (Tin + 2) * st, st, 8), st + 8, 8
        else:
            big = torch.full((B, C_, Tin + 2, Fin + 2), math.nan)
            big[:, :, 1:-1, 1:-1] = data
            strides, off, blk = nets.nchw(C_, Tin + 2, Fin + 2), Fin + 3, 0
        big = dev(big)
        keep.append(big)
        return pb.src(big, C_, *strides, off=off, act=a, blk=blk)

    x0 = randn(B, C0, Tin, Fin) if src is None else src_ref
    if src is None:
        in0 = source(C0, NONE, x0)
    else:
        in0 = pb.src(src[0], C0, *src[2], off=src[1], act=NONE, blk=8)
    x1 = randn(B, C1, Tin, Fin) if C1 else None
    in1 = source(C1, c["act1"], x1) if C1 else None

    K = len(taps) * Cin
    w = {"wk0": (randn(K, Co) * (c["wscale"] / math.sqrt(K))).numpy()}
    if epi == GLU:
        w["wk1"] = (randn(K, Co) * (c["wscale"] / math.sqrt(K))).numpy()
    ref = dict(taps=taps, Wk0=w["wk0"], Wk1=w.get("wk1"), Tout=To, Fout=Fo, sf_in=c["sf_in"], act1=c["act1"], cin1=c["cin1"],
               epi=epi, act_out=c["act"], act_slope=SLOPE if c["act"] == PRELU else 0.0)
    kw = {}
    nb = 2 if epi == GLU else 1
    if c["bias"] == "shared":
        for i in range(nb):
            w["bias%d" % i] = ref["bias%d" % i] = (0.3 * randn(Co)).numpy()
    elif c["bias"] == "item":
        sb = 4 * ((Co + 3) // 4)
        for i in range(nb):
            bt = torch.full((B, sb), math.nan)
            bt[:, :Co] = 0.3 * randn(B, Co)
            ref["bias%d" % i] = bt[:, :Co].clone()
            kw["bias%d" % i], kw["bias%d_sb" % i] = dev(bt), sb
            keep.append(kw["bias%d" % i])
    if c["post"]:
        ps, pt = uni(Co), 0.2 * randn(Co)
        w["post"] = (ps.numpy(), pt.numpy())
        ref["post_scale"], ref["post_shift"] = ps, pt
    if c["xf"]:
        xf = dict(mode=c["xf"], slope0=SLOPE, scale0=uni(Cin).numpy(), shift0=(0.5 + 0.3 * randn(Cin)).numpy())
        if c["xf"] == 2:
            xf.update(slope1=0.1, scale1=uni(Cin).numpy(), shift1=(-0.5 + 0.3 * randn(Cin)).numpy())
        w["xf"] = ref["xf"] = xf
    if c["padrow"]:
        psb = Cin + 2
        pr = torch.full((B, psb), math.nan)
        pr[:, :Cin] = randn(B, Cin)
        ref["padrow"] = pr[:, :Cin].clone()
        kw["padrow"], kw["padrow_sb"] = dev(pr), psb
        keep.append(kw["padrow"])

    strides, cr, off = _layout(c)
    sb, sc_hi, sc_lo, st, sf = strides
    co = np.arange(Co)
    chan = (co // cr) * sc_hi + (co % cr) * sc_lo
    index = (MARGIN + off + np.arange(B)[:, None, None, None] * sb + chan[None, :, None, None]
             + np.arange(To)[None, None, :, None] * st + np.arange(Fo)[None, None, None, :] * sf)
    assert len(np.unique(index)) == index.size
    n = int(index.max()) + 1 + MARGIN + (st + 8 if c["layout"] == "blk8pad" else 0)
    n = (n + 3) // 4 * 4
    buf = torch.full((n,), math.nan, device=device)
    if c["resid"]:
        r = randn(B, Co, To, Fo)
        rbuf = torch.full((n,), math.nan)
        rbuf[torch.from_numpy(index.reshape(-1))] = r.reshape(-1)
        rbuf = dev(rbuf)
        keep.append(rbuf)
        kw["resid"], ref["resid"] = rbuf[MARGIN:], r
    d = pb.gconv(in0=in0, in1=in1, Tin=Tin, Fin=Fin, taps=taps, sf_in=c["sf_in"], W=lambda: w, Cout=Co, epi=epi, act=c["act"],
                 act_slope=ref["act_slope"], cin1=c["cin1"], out=buf[MARGIN:], out_strides=strides, out_off=off, out_cr=cr,
                 B=B, Tout=To, Fout=Fo, s3g=(fam == "gemm"), has_xf=bool(c["xf"]), label=c["id"], **kw)
    out = Built()
    out.case, out.pb, out.desc, out.buf, out.index, out.keep = c, pb, d, buf, index, keep
    out.layout, out.w = (strides, off), w

    def evaluate(dtype, in0_value=None):
        return R.gconv(x0 if in0_value is None else in0_value, x1, dtype=dtype, round_operands="bf16" if d.korder == 4 else None,
                       **ref)

    out.ref = evaluate
    return out


def tensors(built):
    """Every CPU tensor the descriptor may point at (tests/emu.py resolves raw pointers through these)."""
    return built.pb.ctx.all_tensors() + built.keep + [built.buf]


def check_stores(built, buf=None):
    """Returns the kernel's result [B, Cout, Tout, Fout]; asserts that exactly the addressed elements were written."""
    flat = (built.buf if buf is None else buf).detach().cpu()
    idx = torch.from_numpy(built.index.reshape(-1))
    got = flat[idx]
    assert bool(torch.isfinite(got).all()), "%d addressed elements not finite (not stored, or poisoned by a gather beyond the tensor)" % (
        int((~torch.isfinite(got)).sum()))
    rest = torch.ones(flat.numel(), dtype=torch.bool)
    rest[idx] = False
    nanbits = torch.full((1,), math.nan).view(torch.int32)
    assert bool((flat.view(torch.int32)[rest] == nanbits).all()), "stored outside the addressed elements"
    return got.reshape(built.index.shape)


def check_norm(got, ref64, ref32):
    """The tolerance rule of tests/test_gpu_aia_ops.py, unchanged: with e32 the error of the same statement evaluated in
    fp32 on the CPU, rel_l2(result, float64) <= max(4 * e32, 2e-6).  Returns (err, e32)."""
    ref64 = ref64.numpy()
    err = rel_l2(got.numpy(), ref64)
    e32 = rel_l2(ref32.numpy(), ref64)
    bound = max(4 * e32, 2e-6)
    print("result %.3e  fp32 cpu %.3e  bound %.3e  result/e32 %.2f" % (err, e32, bound, err / e32 if e32 else math.inf))
    assert np.isfinite(err) and err <= bound, (err, e32, bound)
    return err, e32
