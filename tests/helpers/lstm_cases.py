"""Case table and descriptor builder shared by tests/test_lstm_refs_host.py (CPU tensors, replayed on tests/emu.py) and
tests/test_gpu_lstm_ops.py (csrc/lstm.hip, csrc/lstmp.hip, csrc/misc.hip: ln_kernel), so that the two cannot drift apart.

A case draws its own natural parameters (``natural``: the state dict of the grouped LSTM, tests/helpers/lstm_refs.py) and
layer-1 input projections (``projections``) from its id, and ``build`` turns them into a pdse_lstm_desc / pdse_glstm_desc /
pdse_glstmp_desc / pdse_ln_desc through the product's own packing (packing.pack_lstm_whh, pack_glstm_wavefront,
pack_glstm_persistent - the functions nets.GcrnPlan calls).  Buffers are laid out for the structural checks:
  * y (and the LayerNorm's out) sits inside a NaN-filled allocation with margins, with gaps between its rows (the frame
    stride is 1024 + 8, the item stride leaves 16 more): after a launch every addressed element is finite and everything
    else is NaN bit for bit;
  * all scratch (hT*, cst*, gx2, part) holds NaN before the launch, and so does the granule buffer of the persistent form,
    which the launch itself zeroes; status is zeroed by the caller, as include/pdse.h documents;
  * rows b >= B of gx / gx1 hold zeros, or NaN with ``pad_nan``.

Parameter regimes (H = 512 and G = 2 are fixed by the kernels):
  n01     weights N(0,1)/sqrt(512), biases and gx O(1); LayerNorm gamma of mixed sign with exact zeros in both 512-chunks,
          beta O(1)
  hot     W_hh times 4: the recurrence dominates and the gates saturate of themselves
  sat     gx columns (and layer 2's bias) at +-100 in each of the four gates in turn: exp overflows to infinity and the
          result must still be the limit value
  tiny    the g gate scaled by 2e-4 so that |c| ~ 1e-4, the cancellation range of tanh_p; judged by the absolute element
          bound alone (one ulp of 1 - 2 rcp(..) is 6e-8, a part in a thousand of such a value, in any fp32 form)
  offset  layer-1 projections that put layer 1's outputs at |mean| >= 0.6 with variance <= 1e-2 over the 1024 features
  flat    the same with variance <= 1e-5, below eps
The pdse_layernorm_f32 cases take their rows from "n01" and "m64" (mean 64, deviation 0.25)."""
import math
import zlib

import numpy as np
import torch

from conftest import pkg, rel_l2
from helpers import lstm_refs as R

G_, H = R.G, R.H
FM = 8                      # elements of NaN in front of and behind an output
Y_ST = 2 * H + 8            # frame stride of y: 8 floats nobody addresses behind every frame
Y_GAP = 16                  # ... and 16 more behind every item
EPS = 1e-5
LAYOUTS = {"il": (2, 1), "cat": (1, H)}          # (y_su, y_sg): stack(dim=-1) + flatten, respectively cat
REGIMES = ("n01", "hot", "sat", "tiny", "offset", "flat")
DISTS = {"n01": (0.0, 1.0), "m64": (64.0, 0.25)}

DEFAULTS = dict(kernel="glstm", B=1, Bp=32, T=7, slices=1, regime="n01", layout="cat",
                N=1024, r=1, blk=0, dist="n01")


def _c(kernel, **kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    c = dict(DEFAULTS, kernel=kernel, **kw)
    if kernel == "ln":
        c["id"] = "ln_B%d_T%d_N%d_r%d_blk%d_%s" % (c["B"], c["T"], c["N"], c["r"], c["blk"], c["dist"])
    else:
        name = kernel + ("_s%d" % c["slices"] if kernel == "glstm" else "")
        bp = "_Bp%d" % c["Bp"] if c["Bp"] % 32 else ""
        c["id"] = "%s_B%d%s_T%d_%s_%s" % (name, c["B"], bp, c["T"], c["regime"], c["layout"])
    return c


def _table(kernel, rows):
    return [_c(kernel, B=B, Bp=Bp, T=T, regime=reg, layout=lay, **({"slices": s} if kernel == "glstm" else {}))
            for (s, B, Bp, T, reg, lay) in rows]


LSTM = _table("lstm", [(0, 1, 32, 1, "n01", "il"), (0, 1, 32, 7, "hot", "cat"), (0, 1, 32, 2, "sat", "cat"),
                       (0, 31, 32, 2, "sat", "il"), (0, 31, 32, 7, "tiny", "cat"), (0, 33, 64, 7, "n01", "cat"),
                       (0, 33, 64, 1, "hot", "il"), (0, 33, 64, 2, "tiny", "il")])
GLSTM = _table("glstm", [(1, 1, 32, 1, "n01", "cat"), (2, 1, 32, 2, "hot", "il"), (1, 31, 32, 3, "sat", "il"),
                         (2, 31, 32, 7, "tiny", "cat"), (1, 32, 32, 7, "offset", "cat"), (2, 32, 32, 33, "flat", "il"),
                         (2, 33, 64, 7, "n01", "cat"), (1, 33, 64, 33, "hot", "cat"), (1, 1, 32, 33, "flat", "cat"),
                         (2, 1, 32, 7, "offset", "il"), (1, 2, 32, 160, "n01", "cat"), (2, 33, 64, 1, "sat", "cat"),
                         (1, 32, 32, 3, "tiny", "il"), (1, 31, 32, 2, "offset", "cat"), (2, 33, 64, 3, "flat", "cat")])
GLSTMP = _table("glstmp", [(0, 1, 32, 1, "n01", "cat"), (0, 2, 32, 2, "hot", "il"), (0, 3, 32, 3, "sat", "cat"),
                           (0, 4, 32, 7, "tiny", "il"), (0, 5, 32, 33, "offset", "cat"), (0, 8, 32, 7, "flat", "cat"),
                           (0, 3, 3, 7, "n01", "il"), (0, 1, 32, 160, "n01", "cat"), (0, 8, 32, 33, "hot", "cat"),
                           (0, 1, 32, 33, "flat", "il"), (0, 2, 32, 7, "offset", "cat"), (0, 5, 32, 2, "sat", "il"),
                           (0, 4, 32, 1, "tiny", "cat"), (0, 8, 32, 3, "n01", "il"), (0, 3, 3, 2, "flat", "cat")])
LN = [_c("ln", B=B, T=T, N=N, r=r, blk=blk, dist=dist) for (B, T, N, r, blk, dist) in [
    (1, 1, 1, 1, 0, "n01"), (1, 1, 1024, 4, 8, "m64"), (1, 3, 63, 4, 0, "m64"), (3, 1, 65, 1, 8, "n01"),
    (1, 5, 1000, 4, 8, "n01"), (5, 1, 1024, 1, 0, "m64"), (1, 3, 1024, 4, 0, "n01"), (3, 1, 1000, 1, 0, "m64"),
    (5, 1, 63, 1, 8, "m64"), (1, 5, 65, 4, 8, "m64"), (1, 3, 1, 4, 8, "m64"), (1, 5, 1024, 1, 8, "n01")]]
ALL = LSTM + GLSTM + GLSTMP + LN


def by_id(cases):
    return [c["id"] for c in cases]


def find(name):
    return next(c for c in ALL if c["id"] == name)


def variant(case, **kw):
    """The case with other sizes and the same id: the same seeds, so the same weights and (per item and frame) projections."""
    return dict(case, **kw)


# ---- natural parameters ---------------------------------------------------------------------------------------------------
_SAT = 100.0


def _sat_pattern():
    """[4H]: unit u with u % 8 == q has gate q at +100, with u % 8 == 4 + q at -100; 0 elsewhere."""
    v = np.zeros((4, H), np.float32)
    for q in range(4):
        v[q, q::8] = _SAT
        v[q, 4 + q::8] = -_SAT
    return v.reshape(-1)


_NAT = {}


def natural(case):
    """The grouped LSTM's state dict for this case: float32 numpy, seeded by the id."""
    key = (case["id"], case["regime"])
    if key in _NAT:
        return _NAT[key]
    reg = case["regime"]
    g = torch.Generator().manual_seed(zlib.crc32(("par:" + case["id"]).encode()))
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).numpy()          # noqa: E731
    p = {}
    for layer in ("lstm_list1", "lstm_list2"):
        for grp in range(G_):
            k = "%s.%d." % (layer, grp)
            p[k + "weight_ih_l0"] = randn(4 * H, H) / math.sqrt(H)
            p[k + "weight_hh_l0"] = randn(4 * H, H) / math.sqrt(H)
            p[k + "bias_ih_l0"], p[k + "bias_hh_l0"] = randn(4 * H), randn(4 * H)
            if reg == "hot":
                p[k + "weight_hh_l0"] *= 4.0
            if reg == "tiny":                                  # the g gate (rows 2H .. 3H) of everything that feeds it
                for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
                    p[k + name][2 * H:3 * H] *= 2e-4
            if reg == "sat" and layer == "lstm_list2":
                p[k + "bias_ih_l0"] += _sat_pattern()
            if reg in ("offset", "flat") and layer == "lstm_list1":
                p[k + "weight_hh_l0"] *= 0.25 if reg == "offset" else 0.01
    for name in ("ln1", "ln2"):
        gam = randn(G_ * H)
        gam[[5, 300, H + 17, H + 400]] = 0.0                   # exact zeros in both 512-chunks; randn gives both signs
        p[name + ".weight"], p[name + ".bias"] = gam, randn(G_ * H)
    _NAT[key] = p
    return p


def projections(case):
    """Layer-1 input projections with both biases, gx1 [G, B, T, 4H] float32: seeded per (id, item), so that item b of a
    batch is the same whatever the batch holds."""
    reg, B, T = case["regime"], case["B"], case["T"]
    first = case.get("first_item", 0)
    out = torch.empty(G_, B, T, 4 * H, dtype=torch.float32)
    for b in range(B):
        g = torch.Generator().manual_seed(zlib.crc32(("gx:%s:%d" % (case["id"], first + b)).encode()))
        out[:, b] = torch.randn(T, G_, 4 * H, generator=g, dtype=torch.float32).transpose(0, 1)
    if reg == "sat":
        out += torch.from_numpy(_sat_pattern())
    if reg == "tiny":
        out[..., 2 * H:3 * H] *= 2e-4
    if reg in ("offset", "flat"):                               # i, f, g, o around 4, 1, 3, 1.4: c -> 3.6, h -> sigmoid(1.4) = 0.80
        base = torch.tensor([4.0, 1.0, 3.0, 1.4]).repeat_interleave(H)
        out = out * (0.3 if reg == "offset" else 0.01) + base
    return out


def ln_params(case):
    g = torch.Generator().manual_seed(zlib.crc32(("par:" + case["id"]).encode()))
    N = case["N"]
    mean, dev = DISTS[case["dist"]]
    x = mean + dev * torch.randn(case["B"], case["T"], N, generator=g, dtype=torch.float32)
    gam = torch.randn(N, generator=g, dtype=torch.float32)
    if N > 8:
        gam[[3, N - 2]] = 0.0
    return x, gam, torch.randn(N, generator=g, dtype=torch.float32)


def ln_strides(case):
    """The two stores nets.GcrnPlan._ln records, at this case's sizes: r = 1 -> [B, C, T] (blk 8: [B, C/8, T, 8]),
    r > 1 -> [B, C, T, r] (blk 8: [B, C/8, T, r, 8]); C = ceil(N / r).  Returns (strides, elements of out)."""
    T, N, r, blk = case["T"], case["N"], case["r"], case["blk"]
    C = -(-N // r)
    lo = r if r > 1 else 1
    if blk:
        Cb = -(-C // 8)
        s = dict(osb=Cb * T * lo * 8, os_hi=T * lo * 8, os_lo=8 if r > 1 else 0, os_t=lo * 8, r=r, blk=8)
        return s, case["B"] * s["osb"]
    s = dict(osb=C * T * lo, os_hi=T * lo, os_lo=1 if r > 1 else 0, os_t=lo, r=r, blk=0)
    return s, case["B"] * s["osb"]


# ---- references, computed once per case and shared ------------------------------------------------------------------------
_REF = {}


def ref(case, dtype):
    """What the launch computes, as [G, B, T, H] (lstm: layer 1 alone; glstm / glstmp: layer 2's output), respectively the
    flat out tensor of the LayerNorm with NaN where nothing is stored.  Cached: callers must leave it unchanged."""
    key = (case["id"], case["B"], case["T"], case.get("first_item", 0), dtype)
    if key not in _REF:
        if case["kernel"] == "ln":
            x, gam, bet = ln_params(case)
            s, n = ln_strides(case)
            _REF[key] = R.ln_store(x, gam, bet, n, s, EPS, dtype)
        elif case["kernel"] == "lstm":
            p = natural(case)
            _REF[key] = R.layer(projections(case), [p["lstm_list1.%d.weight_hh_l0" % g] for g in range(G_)], dtype)
        else:
            res = R.block(projections(case), natural(case), dtype, EPS)
            _REF[key] = torch.stack(torch.chunk(res["y"], G_, dim=-1), 0)
            _REF[key[:-1] + ("y1", dtype)] = res["y1"]
    return _REF[key]


def ref_y1(case, dtype=torch.float64):
    """Layer 1's output [B, T, 1024] (interleaved, in front of LayerNorm 1) of a fused case."""
    ref(case, dtype)
    return _REF[(case["id"], case["B"], case["T"], case.get("first_item", 0), "y1", dtype)]


# ---- buffers --------------------------------------------------------------------------------------------------------------
class Built:
    pass


def _nanbuf(n, device, dtype=torch.float32):
    if dtype == torch.int64:                                   # granules: two NaN patterns per element
        return torch.full((n,), 0x7FC000007FC00000, dtype=torch.int64).to(device)
    return torch.full((n,), math.nan, dtype=dtype).to(device)


def scratch(case, device):
    """The launch's scratch, every byte of it dirty.  Depends on Bp (and on B for the granules) only: a case with another T
    can run on the same one."""
    k, Bp = case["kernel"], case["Bp"]
    if k == "lstm":
        return dict(hT=_nanbuf(2 * G_ * H * Bp, device), cst=_nanbuf(G_ * H * Bp, device))
    if k == "glstm":
        return dict(hT1=_nanbuf(2 * G_ * H * Bp, device), hT2=_nanbuf(2 * G_ * H * Bp, device), cst1=_nanbuf(G_ * H * Bp, device),
                    cst2=_nanbuf(G_ * H * Bp, device), gx2=_nanbuf(2 * G_ * 4 * H * Bp, device),
                    part=_nanbuf(2 * G_ * (H // 8) * Bp * 2, device))
    bq = 1 if case["B"] == 1 else 2 if case["B"] == 2 else 4 if case["B"] <= 4 else 8
    return dict(gran=_nanbuf(4 * 2 * H * bq + 2 * FM, device, torch.int64))


def y_positions(case):
    """Element offsets of y[g][b][t][u] inside the tensor: int64 [G, B, T, H], and the tensor's size."""
    B, T = case["B"], case["T"]
    su, sg = LAYOUTS[case["layout"]]
    sb = T * Y_ST + Y_GAP
    g, b = torch.arange(G_).view(G_, 1, 1, 1), torch.arange(B).view(1, B, 1, 1)
    t, u = torch.arange(T).view(1, 1, T, 1), torch.arange(H).view(1, 1, 1, H)
    return g * sg + b * sb + t * Y_ST + u * su, B * sb


def build(case, device, pad_nan=False, scr=None):
    """The case as one descriptor on ``device``: Built with desc, keep (every tensor a pointer names), out (the NaN-filled
    allocation of y / out), pos (offsets of the addressed elements) and, for the persistent form, status."""
    L, P = pkg("_lib"), pkg("packing")
    c = case
    out = Built()
    out.case = c
    keep = out.keep = []

    def up(a, dtype=np.float32):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)
        keep.append(t)
        return t.data_ptr()

    if c["kernel"] == "ln":
        x, gam, bet = ln_params(c)
        s, n = ln_strides(c)
        d = L.LnDesc()
        d.in_, d.gamma, d.beta = up(x.numpy()), up(gam.numpy()), up(bet.numpy())
        out.out, out.n = _nanbuf(n + 2 * FM, device), n
        keep.append(out.out)
        d.out = out.out.data_ptr() + 4 * FM
        d.osb, d.os_hi, d.os_lo, d.os_t, d.r, d.blk = s["osb"], s["os_hi"], s["os_lo"], s["os_t"], s["r"], s["blk"]
        d.B, d.T, d.N, d.eps = c["B"], c["T"], c["N"], EPS
        out.pos = R.ln_positions(c["B"], c["T"], c["N"], **s)
        out.desc = d
        return out

    B, Bp, T = c["B"], c["Bp"], c["T"]
    p = natural(c)
    gx = projections(c)                                             # [G, B, T, 4H]
    pad = math.nan if pad_nan else 0.0
    out.scr = scr if scr is not None else scratch(c, device)
    keep += list(out.scr.values())
    out.pos, n = y_positions(c)
    out.out, out.n = _nanbuf(n + 2 * FM, device), n
    keep.append(out.out)
    su, sg = LAYOUTS[c["layout"]]
    per = lambda key: [p[key % g] for g in range(G_)]               # noqa: E731
    if c["kernel"] == "lstm":
        full = torch.full((G_, T, 4 * H, Bp), pad, dtype=torch.float32)      # gx [G][T][4H][Bp]
        full[..., :B] = gx.permute(0, 2, 3, 1)
        d = L.LstmDesc()
        d.gx, d.whh = up(full.numpy()), up(P.pack_lstm_whh(per("lstm_list1.%d.weight_hh_l0")))
        d.hT, d.cst = out.scr["hT"].data_ptr(), out.scr["cst"].data_ptr()
    else:
        full = torch.full((G_, T, Bp, 4 * H), pad, dtype=torch.float32)      # gx1 [G][T][Bp][4H]
        full[:, :, :B] = gx.permute(0, 2, 1, 3)
        nat = (per("lstm_list1.%d.weight_hh_l0"), per("lstm_list2.%d.weight_ih_l0"), per("lstm_list2.%d.bias_ih_l0"),
               per("lstm_list2.%d.bias_hh_l0"), per("lstm_list2.%d.weight_hh_l0"), p["ln1.weight"], p["ln1.bias"])
        if c["kernel"] == "glstm":
            d = L.GlstmDesc()
            for k, v in P.pack_glstm_wavefront(*nat).items():
                setattr(d, k, up(v))
            for k in ("hT1", "hT2", "cst1", "cst2", "gx2", "part"):
                setattr(d, k, out.scr[k].data_ptr())
            d.slices = c["slices"]
        else:
            d = L.GlstmpDesc()
            for k, v in P.pack_glstm_persistent(*nat).items():
                setattr(d, k, up(v))
            d.gran = out.scr["gran"].data_ptr() + 8 * FM            # 64 bytes in: 16-byte aligned
            out.status = torch.zeros(4, dtype=torch.int32).to(device)
            keep.append(out.status)
            d.status = out.status.data_ptr()
        d.gx1, d.eps = up(full.numpy()), EPS
    d.y = out.out.data_ptr() + 4 * FM
    d.y_sb, d.y_st, d.y_su, d.y_sg = T * Y_ST + Y_GAP, Y_ST, su, sg
    d.B, d.Bp, d.T, d.H, d.G = B, Bp, T, H, G_
    out.desc = d
    return out


def tensors(built):
    """Every CPU tensor the descriptor may point at (tests/emu.py resolves raw pointers through these)."""
    return built.keep


# ---- reading the results back ---------------------------------------------------------------------------------------------
_NANBITS = torch.full((1,), math.nan).view(torch.int32)


def read(built):
    """The addressed elements of y / out in the shape of ``built.pos``: every one of them finite, everything else in the
    allocation still NaN bit for bit."""
    flat = built.out.detach().cpu()
    idx = built.pos.reshape(-1) + FM
    got = flat[idx]
    bad = int((~torch.isfinite(got)).sum())
    assert bad == 0, "%d addressed elements not finite (not stored, or poisoned)" % bad
    rest = torch.ones(flat.numel(), dtype=torch.bool)
    rest[idx] = False
    assert bool((flat.view(torch.int32)[rest] == _NANBITS).all()), "stored outside the addressed elements"
    return got.reshape(built.pos.shape).clone()


def untouched(built):
    return bool((built.out.detach().cpu().view(torch.int32) == _NANBITS).all())


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ---- tolerances -----------------------------------------------------------------------------------------------------------
def check(what, got, ref64, ref32, regime="n01", factor=4):
    """The project's rule, unchanged: with e32 = rel_l2(the same statement in fp32 on the CPU, float64),
    rel_l2(result, float64) <= max(factor * e32, 2e-6), factor 4; and, because a norm hides one wrong unit, element by element
    max |result - float64| <= max(2 * factor * max |fp32 - float64|, 2e-6) - the factor doubled: a maximum over 1e5 elements
    spreads wider than a norm; the floor absolute: |h| < 1.  Regime "tiny" is judged by the element bound alone.
    Returns (err / bound, element error / element bound)."""
    a = torch.as_tensor(got).double().reshape(-1)
    w, w32 = torch.as_tensor(ref64).double().reshape(-1), torch.as_tensor(ref32).double().reshape(-1)
    sel = ~torch.isnan(w)                                          # the LayerNorm's reference is NaN where nothing is stored
    a, w, w32 = a[sel].numpy(), w[sel].numpy(), w32[sel].numpy()
    assert np.isfinite(a).all(), (what, "NaN or infinity in the result")
    e32 = rel_l2(w32, w)                                           # fp32 on the CPU against float64
    err = rel_l2(a, w)                                             # bound: max(factor * e32, 2e-6)
    bound = max(factor * e32, 2e-6)
    m32 = float(np.abs(w32 - w).max())
    merr = float(np.abs(a - w).max())
    mbound = max(2 * factor * m32, 2e-6)
    line = "%-40s rel_l2 %.3e  fp32 cpu %.3e  bound %.3e  ratio %.3f | max abs %.3e  fp32 cpu %.3e  bound %.3e  ratio %.3f" % (
        what, err, e32, bound, err / bound, merr, m32, mbound, merr / mbound)
    print(line)
    assert merr <= mbound, (what, "element bound", merr, m32, mbound, int(np.abs(a - w).argmax()))
    if regime != "tiny":
        assert err <= bound, (what, "rel_l2", err, e32, bound)
    return err / bound, merr / mbound
