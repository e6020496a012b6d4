"""Case table, descriptor builder and checks shared by tests/test_bglu_refs_host.py (CPU tensors, replayed on tests/emu.py)
and tests/test_gpu_bglu_ops.py (csrc/bglu.hip: bglu_kernel in its five dispatched forms, planes_conv_kernel), so that the
two cannot drift apart.

``build`` makes a synthetic state dict for ONE stage (only the keys that stage reads), hands it to the project's own
packers (packing.bglu_fields, conv_kmat, convT_kmat, compose_stage1, conv_taps, convT_phase_taps, hp_shape, hp_split,
f16_wexp) and fills a pdse_bglu_desc field by field the way nets.EpsNetPlan._bglu / _encoder_planes / _decoders_planes
do, without a plan (``build_stage``; the host file holds it to the descriptors a plan records, for all 15 stages).  The
time-conditioned biases are folded here in float64 as nets.EpsNetPlan._prep_time / _stage_fold fold them (``time_table``:
the slots of one [items, NSLOT * 32] table, NaN where the stage reads nothing).

Kernel contracts the builder honours (a hand-built descriptor that broke one would be at fault, not the kernel):
  * input hp tensors come from packing.hp_split on the host, so their margins are ZERO (out-of-range taps read them),
    rows permuted by packing.hp_par_pos under hp_par; the reference reads packing.hp_join of those same planes, so the
    quantisation of the input is not part of any comparison;
  * nx_hp, both nx_out tensors and nx_add hold B + 1 items and nx_items = B + 1 (item B: the dump target of lanes without
    a position; whatever lands there is unconstrained);
  * every base pointer is a torch allocation of its own, packed weights travel as int16, biases as fp32;
  * inputs stay inside the f16x2 window (|v| < 4094 / 2), and the host file asserts that of every tensor a two-plane launch
    splits (L, R, G, Y, Z).
Buffers for the structural checks: every output sits in an allocation filled with a NaN pattern (0x7fc0 in every uint16 of a
plane tensor: NaN as bf16 and as fp16; float NaN in fp32 tensors) with a guard of the same pattern in front of item 0 and
behind item B.

Geometry (csrc/bglu.hip: launch): P = Tout * Fout positions, tiles = ceil(P / 32), rounds = ceil(tiles / 8), gx =
min(ceil(WGS / B), rounds) workgroups per item, WGS = 256 being launch()'s ``wgs``.  ``kinds`` names what a case reaches;
the host file asserts that every form has every kind at every plane count."""
import math
import zlib

import numpy as np
import torch

from conftest import pkg, rel_l2
from helpers import bglu_refs as R
from helpers import tcm_cases as TC

FM, HM, NAN16 = TC.FM, TC.HM, TC.NAN16
NSLOT = 20                 # nets.EpsNetPlan.NSLOT
SBB = NSLOT * 32
WGS = 256                  # csrc/bglu.hip: launch(): wgs
FORMS = ("enc1", "enc", "enc5", "dec", "dec1")          # the launcher's dispatch keys
DIV = 8                    # np = 1: the divisor of e_b (tests/test_gpu_bglu_ops.py says where it comes from)
SLOPES = (-0.5, 0.0, 0.25, 1.0)
DECS = ("de_real", "de_imag")
# the stage of the network a form stands for in the synthetic state dict: (kind, k)
STAGE = dict(enc1=("en", 1), enc=("en", 2), enc5=("en", 5), dec=("de", 3), dec1=("de", 1))

DEFAULTS = dict(form="enc", np=3, B=2, T=9, Fin=79, params="nominal", ws=None, xscale=1.0, row0=True, temb_items=True,
                gather_items=False, di=0)
# the four weight groups (gather, l_conv / r_conv, conv2, chained) at 2^-10 / 1 / 2^6, with the input scale that keeps the
# activations between them inside the f16x2 window
WS_A = dict(ws=(-10, 6, 0, 6), xscale=2.0 ** 8)
WS_B = dict(ws=(6, -10, 6, -10), xscale=2.0 ** -6)
WS_5 = dict(ws=(6, 0, -10, 0), xscale=2.0 ** -6)         # no chained tile behind conv2: its output leaves as fp32


def _c(name, **kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, id=name, **kw)


def geom(form, Fin):
    """kw, output positions per frame (Fout; decoders: even bins), odd bins (Fout1), bins of the stage's output tensor (Fo)."""
    if form == "enc1":
        return dict(kw=5, Fout=(Fin - 5) // 2 + 1, Fout1=0, Fo=(Fin - 5) // 2 + 1)
    if form in ("enc", "enc5"):
        return dict(kw=3, Fout=(Fin - 3) // 2 + 1, Fout1=0, Fo=(Fin - 3) // 2 + 1)
    kw = 3 if form == "dec" else 5
    Fo = 2 * (Fin - 1) + kw                                   # odd: Fout1 = Fout - 1 always
    return dict(kw=kw, Fout=(Fo + 1) // 2, Fout1=Fo // 2, Fo=Fo)


def launch_geom(c):
    P = c["T"] * geom(c["form"], c["Fin"])["Fout"]
    tiles = (P + 31) // 32
    rounds = (tiles + 7) // 8
    return dict(P=P, tiles=tiles, rounds=rounds, gx=max(1, min((WGS + c["B"] - 1) // c["B"], rounds)))


def kinds(c):
    g = launch_geom(c)
    out = set()
    if g["P"] < 32 and c["T"] == 1:
        out.add("small")                                      # one partial tile, seven idle waves, frame 0 the only frame
    if g["tiles"] > 1 and g["P"] % 32 and g["tiles"] % 8:
        out.add("tiles")
    if g["rounds"] > g["gx"] >= 2 and g["rounds"] % g["gx"] and g["tiles"] % 8:
        out.add("rounds")                                     # workgroups with different trip counts, a partial last round
    if c["B"] == 1:
        out.add("B1")
    return out


def _form_cases(form, npl):
    #            small  tiles  rounds  B1
    fin = dict(enc1=(25, 81, 81, 40), enc=(19, 40, 79, 38), enc5=(9, 40, 79, 19), dec=(4, 19, 38, 9), dec1=(9, 19, 37, 9))[form]
    p = "%snp%d" % (form, npl)
    kw = dict(form=form, np=npl)
    wsa, wsb = (WS_5, WS_5) if form == "enc5" else (WS_A, WS_B)
    return [_c("%s_small_B3_T1_F%d" % (p, fin[0]), B=3, T=1, Fin=fin[0], params="hostile", **kw),
            _c("%s_tiles_B2_T9_F%d" % (p, fin[1]), B=2, T=9, Fin=fin[1], params="hostile", gather_items=form != "enc1", di=1, **wsa, **kw),
            _c("%s_rounds_B128_T14_F%d" % (p, fin[2]), B=128, T=14, Fin=fin[2], **wsb, **kw),
            _c("%s_B1_T5_F%d" % (p, fin[3]), B=1, T=5, Fin=fin[3], params="hostile", row0=False, temb_items=False, di=1, **kw)]


CASES = {npl: [c for f in FORMS for c in _form_cases(f, npl)] for npl in (3, 2, 1)}
ALL = [c for npl in (3, 2, 1) for c in CASES[npl]]


def by_id(cases):
    return [c["id"] for c in cases]


def find(name):
    return next(c for c in ALL if c["id"] == name)


# ---- the synthetic state dict of one stage ----------------------------------------------------------------------------------
def _f32(a):
    """float64 values that fp32 holds exactly: what a state dict carries."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def stage_keys(kind, k, di=0):
    """(key, shape, fan-in or what) of everything stage (kind, k) reads, its chained tiles included."""
    out = []
    lin = lambda p, shape, fan: [(p + ".weight", shape, fan), (p + ".bias", (shape[0],), "b")]      # noqa: E731
    bn = lambda p: [(p + ".weight", (64,), "bn_w"), (p + ".bias", (64,), "bn_b"), (p + ".running_mean", (64,), "bn_m"), (p + ".running_var", (64,), "bn_v")]   # noqa: E731
    kw = 5 if k == 1 else 3
    if kind == "en":
        p = "en.conv%d" % k
        if k == 1:
            out += lin("preprocess.conv", (2, 4, 1, 1), 4) + lin(p + ".conv1", (32, 2, 1, 1), 2) + lin("en.tp1", (2, 512), 512)
        for br in ("l", "r"):
            out += lin("%s.%s" % (p, br), (32, 32, 2, kw), 64 * kw) + lin("%s.%s_conv" % (p, br), (32, 32, 1, 1), 32)
        out += lin(p + ".conv2", (64, 32, 1, 1), 32) + bn("en.en%d.0" % k) + [("en.en%d.1.weight" % k, (1,), "prelu")]
        if k < 5:
            out += lin("en.conv%d.conv1" % (k + 1), (32, 64, 1, 1), 64) + lin("en.tp%d" % (k + 1), (64, 512), 512)
            for de in DECS:
                q = "%s.de%d.0" % (de, k)
                out += [(q + ".conv1.weight", (128, 32, 1, 1), 128), (q + ".conv1.bias", (32,), "b")] + lin(q + ".tp", (128, 512), 512)
        return out
    p = "%s.de%d.0" % (DECS[di], k)
    C2 = 64 if k > 1 else 1
    for br in ("l", "r"):
        out += [("%s.%s.weight" % (p, br), (32, 32, 2, kw), 32 * kw), ("%s.%s.bias" % (p, br), (32,), "b"),
                ("%s.%s_conv.weight" % (p, br), (32, 32, 1, 1), 32), ("%s.%s_conv.bias" % (p, br), (32,), "b")]
    out += [(p + ".conv2.weight", (32, C2, 1, 1), 32), (p + ".conv2.bias", (C2,), "b")]
    if k > 1:
        out += bn("%s.de%d.2" % (DECS[di], k)) + [("%s.de%d.3.weight" % (DECS[di], k), (1,), "prelu")]
        out += [("%s.de%d.0.conv1.weight" % (DECS[di], k - 1), (128, 32, 1, 1), 128)]
    return out


def make_sd(case):
    """Parameters chosen to break it, float64 from a seeded generator (rounded to what fp32 holds): hostile - a PReLU slope from
    SLOPES, BatchNorm scales of mixed sign with two exact zeros, running variances down to 1e-3, O(1) shifts and biases,
    l_conv / r_conv biases of +-30 on every fifth channel (the gate saturates: exp2 overflows, rcp gives 0); ws - the four
    weight groups scaled by powers of two of their own."""
    kind, k = STAGE[case["form"]]
    g = torch.Generator().manual_seed(zlib.crc32(("sd:" + case["id"]).encode()))
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).numpy()          # noqa: E731
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64).numpy()            # noqa: E731
    hostile = case["params"] == "hostile"
    pick = int(torch.randint(0, 4, (1,), generator=g))
    sd = {}
    for key, shape, what in stage_keys(kind, k, case["di"]):
        if what == "b":
            v = randn(*shape) * (1.0 if hostile else 0.1)
        elif what == "bn_w":
            v = 0.4 + 0.8 * rand(*shape)
            if hostile:
                v = v * np.where(rand(*shape) < 0.5, -1.0, 1.0)
                v[[7, 40]] = 0.0
        elif what == "bn_b" or what == "bn_m":
            v = randn(*shape) * (1.0 if hostile else 0.1)
        elif what == "bn_v":
            v = 0.5 + rand(*shape)
            if hostile:
                v[3::16] = 1e-3 * (1.0 + rand(*v[3::16].shape))
        elif what == "prelu":
            v = np.array([SLOPES[pick] if hostile else 0.25])
        else:
            v = randn(*shape) / math.sqrt(what)
        sd[key] = v
    if hostile:
        for key in sd:
            if key.endswith("_conv.bias"):
                sd[key][0::5] = 30.0
                sd[key][2::5] = -30.0
        for key in [k_ for k_ in sd if k_.endswith("running_var")]:       # a small variance under a small weight: the scale stays O(10)
            w = sd[key[:-len("running_var")] + "weight"]
            w[3::16] = np.sign(w[3::16] + 1e-30) * 0.3
    if case["ws"] is not None:
        eG, eLC, eC2, eNX = case["ws"]
        p = ("en.conv%d" % k) if kind == "en" else "%s.de%d.0" % (DECS[case["di"]], k)
        bnp = ("en.en%d.0" % k) if kind == "en" else "%s.de%d.2" % (DECS[case["di"]], k)
        for key in sd:
            if key in (p + ".l.weight", p + ".r.weight", p + ".l.bias", p + ".r.bias"):
                sd[key] = sd[key] * 2.0 ** eG
            elif key in (p + ".l_conv.weight", p + ".r_conv.weight"):
                sd[key] = sd[key] * 2.0 ** eLC
            elif key in (p + ".conv2.weight", p + ".conv2.bias", bnp + ".running_mean", bnp + ".bias"):
                sd[key] = sd[key] * 2.0 ** eC2                    # BatchNorm's mean and shift with it: Y is scaled as a whole
            elif key.endswith("conv1.weight") and not key.startswith(p + "."):
                sd[key] = sd[key] * 2.0 ** eNX
            elif key in ("preprocess.conv.bias", "en.conv1.conv1.bias", "en.tp1.weight", "en.tp1.bias"):
                sd[key] = sd[key] * case["xscale"]                # stage 1: the constant part of h at the scale of the inputs
    return {k_: torch.from_numpy(_f32(v)) for k_, v in sd.items()}


def make_temb(case, B):
    """The time embedding of every item as the network hands it to the projections (silu of something): float64 [items, 512]."""
    g = torch.Generator().manual_seed(zlib.crc32(("temb:" + case["id"]).encode()))
    v = torch.randn(B if case["temb_items"] else 1, 512, generator=g, dtype=torch.float64)
    return (v * torch.sigmoid(v)).numpy()


# ---- time-conditioned biases, folded as nets.EpsNetPlan._prep_time folds them --------------------------------------------------
def _w(sd, k):
    return pkg("packing")._np(sd[k])


def _fold(sd, conv1, tp, transposed):
    """(W1 Wtp [32, 512], b1 + W1 btp [32]) of one stage's conv1 behind its time projection (_stage_fold)."""
    W1 = _w(sd, conv1 + ".weight")[:, :, 0, 0]
    W1 = W1.T if transposed else W1
    return W1 @ _w(sd, tp + ".weight"), _w(sd, conv1 + ".bias") + W1 @ _w(sd, tp + ".bias")


def time_table(sd, temb, kind, k):
    """fp32 [items, NSLOT * 32]: the slots stage (kind, k) reads, NaN everywhere else."""
    tb = np.full((temb.shape[0], SBB), np.nan)

    def put(slot, wf, bf):
        tb[:, 32 * slot:32 * slot + 32] = temb @ wf.T + bf

    if kind == "en" and k == 1:
        wf0, bf0 = _fold(sd, "en.conv1.conv1", "en.tp1", False)
        W1 = _w(sd, "en.conv1.conv1.weight")[:, :, 0, 0]
        bf15 = bf0 + W1 @ _w(sd, "preprocess.conv.bias")        # real rows also carry W1 b_preprocess, the pad row does not
        put(0, wf0, bf0)
        put(15, wf0, bf15)
        for i, br in enumerate(("l", "r")):
            Wg = _w(sd, "en.conv1.%s.weight" % br)
            S0, S1 = Wg[:, :, 0].sum(-1), Wg[:, :, 1].sum(-1)
            bg = _w(sd, "en.conv1.%s.bias" % br)
            put(16 + 2 * i, (S0 + S1) @ wf0, (S0 + S1) @ bf15 + bg)
            put(17 + 2 * i, (S0 + S1) @ wf0, S0 @ bf0 + S1 @ bf15 + bg)
    if kind == "en" and k < 5:
        put(k, *_fold(sd, "en.conv%d.conv1" % (k + 1), "en.tp%d" % (k + 1), False))
        for di, de in enumerate(DECS):
            put(5 + 5 * di + (5 - k), *_fold(sd, "%s.de%d.0.conv1" % (de, k), "%s.de%d.0.tp" % (de, k), True))
    return tb.astype(np.float32)


def natural(sd, kind, k, di, temb, gather_bias=None):
    """The natural parameters bglu_refs takes, float64, straight from the state dict - conv1 biases with the projected time
    embedding behind them computed as the modules do (project, add, convolve), not as the table folds them."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))          # noqa: E731
    w = lambda key: _w(sd, key)                                                  # noqa: E731
    tr = kind == "de"
    p_ = ("en.conv%d" % k) if kind == "en" else "%s.de%d.0" % (DECS[di], k)
    m = (lambda a: a[:, :, 0, 0].T) if tr else (lambda a: a[:, :, 0, 0])         # ConvTranspose2d keeps [in, out]
    p = dict(Wl=t(w(p_ + ".l.weight")), Wr=t(w(p_ + ".r.weight")), bl=t(w(p_ + ".l.bias")), br=t(w(p_ + ".r.bias")),
             Wlc=t(m(w(p_ + ".l_conv.weight"))), Wrc=t(m(w(p_ + ".r_conv.weight"))), blc=t(w(p_ + ".l_conv.bias")), brc=t(w(p_ + ".r_conv.bias")),
             W2=t(m(w(p_ + ".conv2.weight"))), b2=t(w(p_ + ".conv2.bias")), slope=1.0, nx=[])
    if gather_bias is not None:
        p["bl"], p["br"] = t(gather_bias[0]), t(gather_bias[1])
    if kind == "en" or k > 1:
        bnp = ("en.en%d.0" % k) if kind == "en" else "%s.de%d.2" % (DECS[di], k)
        p["bn"] = tuple(t(w(bnp + s_)) for s_ in (".weight", ".bias", ".running_mean", ".running_var"))
        p["slope"] = float(w(("en.en%d.1.weight" % k) if kind == "en" else "%s.de%d.3.weight" % (DECS[di], k))[0])

    def conv1_bias(conv1, tp, transposed):
        W1 = w(conv1 + ".weight")[:, :, 0, 0]
        proj = temb @ w(tp + ".weight").T + w(tp + ".bias")                      # Linear(512, Cin)
        return proj @ (W1 if transposed else W1.T) + w(conv1 + ".bias")

    if kind == "en" and k == 1:
        p.update(Wpre=t(w("preprocess.conv.weight")[:, :, 0, 0]), bpre=t(w("preprocess.conv.bias")), W1=t(w("en.conv1.conv1.weight")[:, :, 0, 0]),
                 bh=t(conv1_bias("en.conv1.conv1", "en.tp1", False)))
    if kind == "en" and k < 5:
        p["nx"].append(dict(W=t(w("en.conv%d.conv1.weight" % (k + 1))[:, :, 0, 0]), bias=t(conv1_bias("en.conv%d.conv1" % (k + 1), "en.tp%d" % (k + 1), False))))
        for de in DECS:
            q = "%s.de%d.0" % (de, k)
            p["nx"].append(dict(W=t(w(q + ".conv1.weight")[:, :, 0, 0].T[:, 64:]), bias=t(conv1_bias(q + ".conv1", q + ".tp", True)[:, :])))
    if kind == "de" and k > 1:
        p["nx"].append(dict(W=t(w("%s.de%d.0.conv1.weight" % (DECS[di], k - 1))[:, :, 0, 0].T[:, :64]), bias=t(np.zeros((1, 32)))))
    return p


# ---- buffers ------------------------------------------------------------------------------------------------------------------
class Built:
    pass


def _u16buf(n, device, inner=None):
    big = np.full(n + 2 * HM, NAN16, np.uint16)
    if inner is not None:
        big[HM:HM + n] = np.asarray(inner, np.uint16).reshape(-1)
    return torch.from_numpy(big.view(np.int16)).to(device)


def par_store(hp):
    """hp in natural bin order -> rows stored split by parity (natural[i] = stored[hp_par_pos[i]])."""
    out = np.zeros_like(hp)
    out[:, :, :, :, pkg("packing").hp_par_pos(hp.shape[4]), :] = hp
    return out


def skip_store(x, Fh, items):
    """[B, 32, T, F] -> the skip layout [items][8 groups][T][F][4] (NaN in the items behind B), bins split by parity when Fh."""
    B, _, T, F_ = x.shape
    out = np.full((items, 8, T, F_, 4), np.nan, np.float32)
    pos = (np.arange(F_) & 1) * Fh + (np.arange(F_) >> 1) if Fh else np.arange(F_)
    out[:B][:, :, :, pos, :] = np.asarray(x, np.float32).reshape(B, 8, 4, T, F_).transpose(0, 1, 3, 4, 2)
    return out


def skip_load(a, Fh):
    """Inverse of skip_store on [B, 8, T, F, 4]."""
    B, _, T, F_, _ = a.shape
    pos = (np.arange(F_) & 1) * Fh + (np.arange(F_) >> 1) if Fh else np.arange(F_)
    return np.ascontiguousarray(a[:, :, :, pos, :].transpose(0, 1, 4, 2, 3)).reshape(B, 32, T, F_)


def build_stage(sd, kind, k, di, B, T, Fin, npl, device, temb, row0=True, gather_items=False, xscale=1.0, seed=0, parity=True):
    """One stage of the network as one pdse_bglu_desc on ``device``: field by field what nets.EpsNetPlan._bglu records for it."""
    L, P = pkg("_lib"), pkg("packing")
    form = ("enc1" if k == 1 else "enc5" if k == 5 else "enc") if kind == "en" else ("dec1" if k == 1 else "dec")
    gm = geom(form, Fin)
    kw, Fo = gm["kw"], gm["Fo"]
    g = torch.Generator().manual_seed(seed)
    out = Built()
    keep = out.keep = []
    out.form, out.B, out.T, out.np, out.Fin, out.Fo, out.kind, out.k, out.di, out.sd_ = form, B, T, npl, Fin, Fo, kind, k, di, sd

    def up(a, dtype=np.float32):
        t_ = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)
        keep.append(t_)
        return t_

    # ---- weight side: the plan's make() of this stage
    p_ = ("en.conv%d" % k) if kind == "en" else "%s.de%d.0" % (DECS[di], k)
    chained = (kind == "en" and k < 5) or (kind == "de" and k > 1)
    if kind == "en":
        kk, taps = P.conv_taps(2, kw, 1)
        nxw = []
        if chained:
            nxw = [_w(sd, "en.conv%d.conv1.weight" % (k + 1))[:, :, 0, 0]] + [_w(sd, "%s.de%d.0.conv1.weight" % (de, k))[:, :, 0, 0].T[:, 64:] for de in DECS]
        if k == 1:
            gather = dict(zip(("w0", "w1"), P.compose_stage1(sd, p_, kk)))
        else:
            gather = dict(w0=P.conv_kmat(sd[p_ + ".l.weight"], kk), w1=P.conv_kmat(sd[p_ + ".r.weight"], kk))
        fields = P.bglu_fields(sd, p_, False, 64, "en.en%d.0" % k, gather, nxw, npl, k > 1)
        p1mask, C2, sf_in = 0, 64, 2
    else:
        kk0, taps = P.convT_phase_taps(2, kw, 0)
        kk1, taps1 = P.convT_phase_taps(2, kw, 1)
        p1mask = sum(1 << taps.index(tp) for tp in taps1)
        C2, sf_in = (64 if k > 1 else 1), 1
        gather = dict(w0=P.convT_kmat(sd[p_ + ".l.weight"], kk0), w1=P.convT_kmat(sd[p_ + ".r.weight"], kk0),
                      w2=P.convT_kmat(sd[p_ + ".l.weight"], kk1), w3=P.convT_kmat(sd[p_ + ".r.weight"], kk1))
        nxw = [_w(sd, "%s.de%d.0.conv1.weight" % (DECS[di], k - 1))[:, :, 0, 0].T[:, :64]] if k > 1 else []
        fields = P.bglu_fields(sd, p_, True, C2, "%s.de%d.2" % (DECS[di], k) if k > 1 else None, gather, nxw, npl, True)
    gather_bias = None
    if gather_items and not (kind == "en" and k == 1):          # a bias row per item where the network has one for all
        gather_bias = [np.asarray(fields[f], np.float64)[None] * (1.0 + 0.5 * torch.randn(B, 32, generator=g, dtype=torch.float64).numpy()) for f in ("bias0", "bias1")]
        gather_bias = [_f32(v) for v in gather_bias]
        fields["bias0"], fields["bias1"] = gather_bias
    out.fields = fields
    d = L.BgluDesc()
    for key, v in fields.items():
        setattr(d, key, (up(v.view(np.int16), np.int16) if v.dtype == np.uint16 else up(v)).data_ptr() if isinstance(v, np.ndarray) else v)
    if gather_bias is not None:
        d.bias_sb = 32
    # ---- inputs
    if form == "enc1":
        out.x = [torch.randn(B, 2, T, Fin, generator=g, dtype=torch.float32) * xscale for _ in range(2)]
        out.xbuf = [TC._fbuf(x, B * 2 * T * Fin, device) for x in out.x]
        keep += out.xbuf
        s = (2 * T * Fin, T * Fin, Fin, 1)
        d.x0, d.x1 = (L.Src(TC.fptr(b_), *s, 2, L.ACT_NONE, 0, 0) for b_ in out.xbuf)
        out.h_in = None
    else:
        h = torch.randn(B, 32, T, Fin, generator=g, dtype=torch.float32) * xscale
        hp = P.hp_split(h.numpy(), npl)
        out.h_in = torch.from_numpy(P.hp_join(hp))                       # what the planes hold: the reference's input
        out.hp_in = par_store(hp) if (kind == "en" and parity) else hp
        shp = P.hp_shape(B + 1, T, Fin, npl)
        out.hpbuf = _u16buf(out.hp_in.size, device, out.hp_in)
        keep.append(out.hpbuf)
        d.hp, d.hp_sb, d.hp_Tp, d.hp_Fp, d.hp_t0, d.hp_f0 = TC.hptr(out.hpbuf), int(np.prod(shp[1:])), shp[1], shp[4], P.HP_T0, P.HP_F0
        d.hp_par = 1 if (kind == "en" and parity) else 0
    d.Tin, d.Fin = T, Fin
    d.ntaps, d.sf_in = len(taps), sf_in
    for i, (dt_, df_) in enumerate(taps):
        d.tap_dt[i], d.tap_df[i] = int(dt_), int(df_)
    d.p1mask, d.Fout1 = p1mask, gm["Fout1"]
    d.B, d.Tout, d.Fout, d.np = B, T, gm["Fout"], npl
    # ---- time-conditioned biases
    out.temb = temb
    tsb = SBB if temb.shape[0] > 1 else 0
    if kind == "en" and k < 5:
        out.tb = up(time_table(sd, temb, kind, k))
        slot = lambda s_: out.tb.data_ptr() + 4 * 32 * s_                 # noqa: E731
        if k == 1:
            d.bias0, d.bias1, d.bias0_t0, d.bias1_t0, d.bias_sb = slot(16), slot(18), slot(17), slot(19), tsb
    d.slope = 1.0 if (kind == "de" and k == 1) else float(_w(sd, ("en.en%d.1.weight" % k) if kind == "en" else "%s.de%d.3.weight" % (DECS[di], k))[0])
    d.C2 = C2
    # ---- outputs
    d.nx_n = (1 + (2 if kind == "en" else 0)) if chained else 0
    d.nx_items = B + 1
    out.add = None
    if chained:
        shp = P.hp_shape(B + 1, T, Fo, npl)
        out.nx_shape = shp
        out.nxbuf = _u16buf(int(np.prod(shp)), device)
        keep.append(out.nxbuf)
        d.nx_hp, d.nx_hp_sb, d.nx_Tp, d.nx_Fp, d.nx_t0, d.nx_f0 = TC.hptr(out.nxbuf), int(np.prod(shp[1:])), shp[1], shp[4], P.HP_T0, P.HP_F0
        d.skip_Fh = (Fo + 1) // 2 if parity else 0
        sk = (32 * T * Fo, 4 * T * Fo, 4 * Fo, 4)
        if kind == "en":
            d.nx_row0, d.nx_par = (1 if row0 else 0), (1 if parity else 0)
            out.skbuf = [TC._fbuf(None, (B + 1) * 32 * T * Fo, device) for _ in range(2)]
            keep += out.skbuf
            for i in range(2):
                d.nx_out[i] = TC.fptr(out.skbuf[i])
                d.nx_sb[i], d.nx_sc[i], d.nx_st[i], d.nx_sf[i] = sk
            for i, s_ in enumerate((k, 5 + (5 - k), 10 + (5 - k))):
                d.nx_bias[i], d.nx_bias_sb[i] = slot(s_), tsb
        else:
            out.add = torch.randn(B, 32, T, Fo, generator=g, dtype=torch.float32)              # O(1) skip addends
            out.addbuf = TC._fbuf(skip_store(out.add.numpy(), d.skip_Fh, B + 1), (B + 1) * 32 * T * Fo, device)
            out.zero32 = up(np.zeros(32))
            keep.append(out.addbuf)
            d.nx_add, d.add_sb, d.add_sc, d.add_st, d.add_sf = (TC.fptr(out.addbuf),) + sk
            d.nx_bias[0], d.nx_bias_sb[0] = out.zero32.data_ptr(), 0
    elif kind == "en":
        out.outbuf = TC._fbuf(None, B * 64 * Fo * T, device)                                   # stored [B, 64, F, T]
        d.out, d.out_sb, d.out_sc, d.out_st, d.out_sf = TC.fptr(out.outbuf), 64 * Fo * T, Fo * T, 1, T
    else:
        out.outbuf = TC._fbuf(None, B * 2 * T * Fo, device)                                    # [B, 2 decoders, T, F]
        d.out, d.out_sb, d.out_sc, d.out_st, d.out_sf, d.out_off = TC.fptr(out.outbuf), 2 * T * Fo, T * Fo, Fo, 2, di * T * Fo
    if not chained:
        keep.append(out.outbuf)
    out.desc = d
    out.p = natural(sd, kind, k, di, temb, gather_bias)

    def ref(dtype, rnd=False):
        key = (dtype, rnd)
        if key not in out._refs:
            if kind == "en":
                r = R.encoder(out.p, dtype, h=out.h_in, rnd=rnd) if k > 1 else R.encoder(out.p, dtype, x0=out.x[0], x1=out.x[1], rnd=rnd)
            else:
                r = R.decoder(out.p, out.h_in, dtype, rnd=rnd, add=out.add)
            out._refs[key] = r
        return out._refs[key]

    out._refs = {}
    out.ref = ref
    return out


def build(case, device):
    """The case as one descriptor on ``device``: Built with desc, the buffers, keep (every tensor a pointer names), ref(dtype,
    rnd=False) -> what bglu_refs says the launch computes."""
    c = case
    kind, k = STAGE[c["form"]]
    sd = make_sd(c)
    b = build_stage(sd, kind, k, c["di"], c["B"], c["T"], c["Fin"], c["np"], device, make_temb(c, c["B"]), row0=c["row0"],
                    gather_items=c["gather_items"], xscale=c["xscale"], seed=zlib.crc32(c["id"].encode()))
    b.case, b.sd = c, sd
    return b


def tensors(built):
    return built.keep


# ---- reading the results back --------------------------------------------------------------------------------------------------
def _inner_f(buf, n):
    """The n floats between the guards of a float allocation; the guards still NaN bit for bit."""
    flat = buf.detach().cpu()
    nanbits = torch.full((1,), math.nan).view(torch.int32)
    edge = torch.cat([flat[:FM], flat[FM + n:]]).view(torch.int32)
    assert flat.numel() == n + 2 * FM and bool((edge == nanbits).all()), "stored outside the tensor"
    return flat[FM:FM + n]


def _is_nan_pattern(t):
    return bool((t.contiguous().view(torch.int32) == torch.full((1,), math.nan).view(torch.int32)).all())


def read_planes(b):
    """The chained plane tensor of items 0 .. B-1 as float32 [B, 32, T, F]: guards and margins (the frame above frame 0, HP_F0
    bins either side - under nx_par the same set through hp_par_pos) hold the pattern bit for bit, every own element was
    overwritten and is finite; with nx_row0 the pad frame is hp_split of the broadcast conv1 bias, bit for bit.  Item B (the
    dump target) is unconstrained."""
    P = pkg("packing")
    d, B, T = b.desc, b.B, b.T
    shp = b.nx_shape
    n = int(np.prod(shp))
    raw = b.nxbuf.detach().cpu().numpy().view(np.uint16)
    assert (raw[:HM] == NAN16).all() and (raw[HM + n:] == NAN16).all(), "stored outside the plane tensor"
    hp = raw[HM:HM + n].reshape(shp)[:B]
    if d.nx_par:
        hp = hp.take(P.hp_par_pos(shp[4]), axis=4)                        # natural bin order
    F_ = shp[4] - 2 * P.HP_F0
    own = hp[:, P.HP_T0:, :, :, P.HP_F0:P.HP_F0 + F_, :]
    assert (own != NAN16).all(), "%d own uint16 of nx_hp not overwritten" % int((own == NAN16).sum())
    margin = np.ones(hp.shape, bool)
    margin[:, P.HP_T0:, :, :, P.HP_F0:P.HP_F0 + F_, :] = False
    if d.nx_row0:
        margin[:, P.HP_T0 - 1, :, :, P.HP_F0:P.HP_F0 + F_, :] = False
        bias = b.tb.detach().cpu().numpy()[:, 32 * b.k:32 * b.k + 32]
        want = P.hp_split(np.broadcast_to(bias.reshape(-1, 32, 1, 1), (bias.shape[0], 32, 1, F_)), b.np)[:, P.HP_T0, :, :, P.HP_F0:P.HP_F0 + F_, :]
        got = hp[:, P.HP_T0 - 1, :, :, P.HP_F0:P.HP_F0 + F_, :]
        assert (got == np.broadcast_to(want, got.shape)).all(), "pad frame is not hp_split of the conv1 bias"
    assert (hp[margin] == NAN16).all(), "%d margin uint16 of nx_hp written" % int((hp[margin] != NAN16).sum())
    clean = np.where(margin | (hp == NAN16), np.uint16(0), hp)
    if d.nx_row0:
        clean[:, P.HP_T0 - 1] = 0
    v = P.hp_join(clean)
    assert np.isfinite(v).all(), "own elements of nx_hp not finite"
    return torch.from_numpy(v)


def read_skip(b, i):
    d, B, T, Fo = b.desc, b.B, b.T, b.Fo
    a = _inner_f(b.skbuf[i], (B + 1) * 32 * T * Fo).reshape(B + 1, 8, T, Fo, 4)[:B]
    assert bool(torch.isfinite(a).all()), "skip tensor %d: %d elements not stored" % (i, int((~torch.isfinite(a)).sum()))
    return torch.from_numpy(skip_load(a.numpy(), d.skip_Fh))


def read_out(b):
    """enc5: [B, 64, T, F] from its [B, 64, F, T] storage; dec1: [B, T, F] of decoder di, the other decoder's channel untouched."""
    B, T, Fo = b.B, b.T, b.Fo
    if b.form == "enc5":
        return TC.read_f(b.outbuf, (B, 64, Fo, T)).permute(0, 1, 3, 2).contiguous()
    a = _inner_f(b.outbuf, B * 2 * T * Fo).reshape(B, 2, T, Fo)
    assert _is_nan_pattern(a[:, 1 - b.di]), "the other decoder's channel of out was written"
    assert bool(torch.isfinite(a[:, b.di]).all()), "out: elements not stored"
    return a[:, b.di].clone()


def inputs_unchanged(b):
    """hp / x0 / x1 / nx_add, every uploaded weight and constant operand (the per-item gather biases among them), the time table
    and the zero bias row of the decoders are bit-identical to what was uploaded."""
    if b.form == "enc1":
        ok = all(TC.read_f(buf, tuple(x.shape)).equal(x) for buf, x in zip(b.xbuf, b.x))
    else:
        raw = b.hpbuf.detach().cpu().numpy().view(np.uint16)
        n = b.hp_in.size
        ok = bool((raw[:HM] == NAN16).all() and (raw[HM + n:] == NAN16).all() and (raw[HM:HM + n] == b.hp_in.reshape(-1)).all())
    if b.add is not None:
        a = _inner_f(b.addbuf, (b.B + 1) * 32 * b.T * b.Fo).reshape(b.B + 1, 8, b.T, b.Fo, 4)
        ok = ok and _is_nan_pattern(a[b.B]) and bool(torch.from_numpy(skip_load(a[:b.B].numpy(), b.desc.skip_Fh)).equal(b.add))
    for key, v in b.fields.items():
        if isinstance(v, np.ndarray):
            t_ = next(t_ for t_ in b.keep if t_.data_ptr() == getattr(b.desc, key))
            want = v.view(np.int16) if v.dtype == np.uint16 else np.ascontiguousarray(v, np.float32)
            ok = ok and t_.detach().cpu().numpy().tobytes() == want.tobytes()
    if hasattr(b, "tb"):              # the time table behind bias0 / bias1 (+ _t0) of stage 1 and every nx_bias of the encoders
        ok = ok and b.tb.detach().cpu().numpy().tobytes() == time_table(b.sd_, b.temb, b.kind, b.k).tobytes()
    if hasattr(b, "zero32"):
        ok = ok and not b.zero32.detach().cpu().numpy().view(np.uint32).any()
    return ok


def outputs_untouched(b):
    """Every output allocation still holds its pattern (a refused descriptor launched nothing)."""
    ok = True
    if hasattr(b, "nxbuf"):
        ok = ok and bool((b.nxbuf.detach().cpu().numpy().view(np.uint16) == NAN16).all())
    for buf in getattr(b, "skbuf", []) + ([b.outbuf] if hasattr(b, "outbuf") else []):
        ok = ok and TC.untouched_f(buf)
    return ok


# ---- the checks: structure (the readers above) and values -------------------------------------------------------------------------
def outputs(b):
    """[(name, result read back, key into the reference)] of everything the launch writes."""
    if b.form in ("enc5", "dec1"):
        return [("out", read_out(b), "Y" if b.form == "enc5" else "out")]
    out = [("nx_hp", read_planes(b), 0)]
    if b.kind == "en":
        out += [("nx_out[%d]" % i, read_skip(b, i), i + 1) for i in range(2)]
    return out


def _pick(r, key):
    return r[key] if isinstance(key, str) else r["Z"][key]


def verify(b, rows=None):
    """Every check of one finished launch (the GPU file after the kernel, the host file after the emulator).
    np 3 / 2: the fp32 rule (tcm_cases.check_fp32) for every output tensor.  np 1: fp32 outputs by tcm_cases.check_bf16 with the
    divisor DIV; the plane output element by element (tcm_cases.check_elems_bf16) against the chained conv1 of the rounding
    reference in float64 - bf16 weights on the reference's own bf16-rounded Y, as the kernel multiplies them (tcm_cases.
    check_hs_bf16 does the same), the RESULT left unrounded: the one rounding the rule allows for is the kernel's last.  The
    kernel's own Y never reaches memory, so a rounding of Y that the kernel's fp32 noise carried across a tie is part of what the
    element rule has to absorb here.
    rows: a list that receives (case, tensor, error, bound, error / bound, what) for the margins table."""
    c = b.case
    rnd = b.np == 1
    r64, r32 = b.ref(torch.float64, rnd), b.ref(torch.float32, rnd)
    plain = b.ref(torch.float64) if rnd else None
    for name, got, key in outputs(b):
        what = "%s %s" % (c["id"], name)
        ref64, ref32 = _pick(r64, key), _pick(r32, key)
        if not rnd:
            err, e32 = TC.check_fp32(what, got, ref64, ref32, None)
            bound = max(4 * e32, 2e-6)
            if rows is not None:
                rows.append((c["id"], name, err, bound, err / bound, "fp32 rule, e32 %.3e" % e32))
        elif name == "nx_hp":
            worst = TC.check_elems_bf16(what, TC.own(got, None), TC.own(ref64, None), TC.own(ref32, None))
            print("%s: worst |diff| / (2^-8 |ref| + allowance) %.3f" % (what, worst))
            if rows is not None:
                rows.append((c["id"], name, worst, 1.0, worst, "element rule"))
        else:
            err, e_b, e32 = TC.check_bf16(what, got, ref64, ref32, _pick(plain, key), None, div=DIV)
            if rows is not None:
                rows.append((c["id"], name, err, max(4 * e32, e_b / DIV), err / max(4 * e32, e_b / DIV), "e_b %.3e err/e_b %.4f e32r %.3e" % (e_b, err / e_b, e32)))
    assert inputs_unchanged(b), "%s: an input changed" % c["id"]


# ---- planes_conv (decoder stage 5's conv1 on the fp32 matrix cores) ----------------------------------------------------------------
PC_CASES = [dict(id="pc_np%d_nd%d_c%d_%d_T%d_B%d_%s" % (npl, nd, c0, c1, T, B, "bias" if bias else "nobias"), np=npl, nd=nd, cin0=c0, cin1=c1, T=T, B=B, bias=bias)
            for npl in (3, 2, 1) for nd in (1, 2) for c0, c1 in ((32, 0), (64, 0), (64, 32), (64, 64)) for T in (1, 9, 33) for B in (1, 3) for bias in (True, False)]


def build_pc(case, device):
    """pdse_planes_desc with w: source strides as the net's ([B, C, 4, T] storage: in_st = 1, in_sf = T), both sources in
    allocations of the same batch stride (channels behind a source's own hold NaN), NaN-pattern plane outputs."""
    L, P = pkg("_lib"), pkg("packing")
    c = case
    B, T, npl, nd, c0, c1 = c["B"], c["T"], c["np"], c["nd"], c["cin0"], c["cin1"]
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    out = Built()
    keep = out.keep = []
    out.case = c
    Cm = max(c0, c1)
    d = L.PlanesDesc()
    out.xs, out.xbuf = [], []
    for ci in (c0, c1):
        if ci == 0:
            continue
        x = torch.randn(B, ci, T, 4, generator=g, dtype=torch.float32)
        st = torch.full((B, Cm, 4, T), math.nan)
        st[:, :ci] = x.permute(0, 1, 3, 2)
        out.xs.append(x)
        out.xbuf.append(TC._fbuf(st, B * Cm * 4 * T, device))
    keep += out.xbuf
    d.in_ = TC.fptr(out.xbuf[0])
    if c1:
        d.in1 = TC.fptr(out.xbuf[1])
    d.in_sb, d.in_sc, d.in_st, d.in_sf = Cm * 4 * T, 4 * T, 1, T
    shp = P.hp_shape(B + 1, T, 4, npl)
    out.shape = shp
    out.hpbuf = [_u16buf(int(np.prod(shp)), device) for _ in range(nd)]
    keep += out.hpbuf
    d.hp = TC.hptr(out.hpbuf[0])
    if nd == 2:
        d.hp1 = TC.hptr(out.hpbuf[1])
    d.hp_sb, d.hp_Tp, d.hp_Fp, d.hp_t0, d.hp_f0 = int(np.prod(shp[1:])), shp[1], shp[4], P.HP_T0, P.HP_F0
    d.B, d.T, d.F, d.np, d.cin0, d.cin1, d.nd = B, T, 4, npl, c0, c1, nd
    out.W = [_f32(torch.randn(32, c0 + c1, generator=g, dtype=torch.float64).numpy() / math.sqrt(c0 + c1)) for _ in range(nd)]
    out.bias = [_f32(torch.randn(B, 32, generator=g, dtype=torch.float64).numpy()) if c["bias"] else None for _ in range(nd)]
    out.wt, out.bt = [], []
    for i in range(nd):
        wt = torch.from_numpy(np.ascontiguousarray(out.W[i].T, np.float32)).to(device)           # k-major [cin, 32]
        out.wt.append(wt)
        d.w[i] = wt.data_ptr()
        if c["bias"]:
            bt = torch.full((B, SBB), math.nan)
            bt[:, 32 * i:32 * i + 32] = torch.from_numpy(out.bias[i]).float()
            out.bt.append(bt.to(device))
            d.bias[i] = out.bt[-1].data_ptr() + 4 * 32 * i
    d.bias_sb = SBB if c["bias"] else 0
    keep += out.wt + out.bt
    out.desc = d
    out.ref = lambda dtype: R.conv1_cat(out.xs, out.W, out.bias, dtype)
    return out


def read_pc(b, i, strict=True):
    """Planes of weight set i, items 0 .. B-1, as float32 [B, 32, T, 4]: guards, the dump item, the frame above frame 0 and the
    bins either side hold the pattern bit for bit; every own element was overwritten."""
    P = pkg("packing")
    shp = b.shape
    n = int(np.prod(shp))
    raw = b.hpbuf[i].detach().cpu().numpy().view(np.uint16)
    assert (raw[:HM] == NAN16).all() and (raw[HM + n:] == NAN16).all(), "stored outside the plane tensor"
    hp = raw[HM:HM + n].reshape(shp)
    margin = np.ones(hp.shape, bool)
    margin[:b.case["B"], P.HP_T0:, :, :, P.HP_F0:P.HP_F0 + 4, :] = False
    assert not strict or (hp[margin] == NAN16).all(), "planes_conv: margins written"
    assert (hp[~margin] != NAN16).all(), "planes_conv: own elements left"
    v = P.hp_join(np.where(margin, np.uint16(0), hp)[:b.case["B"]])
    assert np.isfinite(v).all()
    return torch.from_numpy(v)


def verify_pc(b, rows=None, strict=True):
    c = b.case
    r64, r32 = b.ref(torch.float64), b.ref(torch.float32)
    for i in range(c["nd"]):
        got = read_pc(b, i, strict)
        what = "%s hp%d" % (c["id"], i)
        if c["np"] == 1:          # the fp32 accumulator, rounded once to bf16: the element rule
            worst = TC.check_elems_bf16(what, TC.own(got, None), TC.own(r64[i], None), TC.own(r32[i], None))
            if rows is not None:
                rows.append((c["id"], "hp%d" % i, worst, 1.0, worst, "element rule"))
        else:
            err, e32 = TC.check_fp32(what, got, r64[i], r32[i], None)
            if rows is not None:
                rows.append((c["id"], "hp%d" % i, err, max(4 * e32, 2e-6), err / max(4 * e32, 2e-6), "fp32 rule, e32 %.3e" % e32))
    for buf, x in zip(b.xbuf, b.xs):                      # the sources stay as they were
        st = _inner_f(buf, buf.numel() - 2 * FM).reshape(c["B"], -1, 4, c["T"])
        assert st[:, :x.shape[1]].permute(0, 1, 3, 2).equal(x)
