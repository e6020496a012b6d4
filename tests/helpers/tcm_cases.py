"""Case table and descriptor builder shared by tests/test_tcm_refs_host.py (CPU tensors, replayed on tests/emu.py) and
tests/test_gpu_tcm_ops.py (csrc/tcm.hip, csrc/tcm2.hip), so that the two cannot drift apart.

A case chooses every slope, scale, shift and bias of a block itself (``params``), and ``build`` turns the natural
parameters into a pdse_tcm_desc / pdse_tcm2_desc / pdse_tcm2s_desc with the packers, in the way
packing.tcm_fields / packing.tcm2_fields do for nets.EpsNetPlan._residual_fused / _residual_split (tcm_fields / tcm2_fields
here; the host file holds the two to byte identity on a synthetic DiffUNet1).  Buffers are laid out for the structural checks of the GPU file:
  * x, x_out, h, h_out sit inside allocations whose margins hold NaN: after a launch every addressed element is finite
    and the margins are NaN bit for bit;
  * an hs tensor keeps its 64 zero frames on either side (a tap outside [0, T) is an address there, not a select), the
    allocation around it holds a NaN bit pattern (0x7fc0: NaN as bf16 and as fp16), and so do the own frames of hs_out
    before the launch: afterwards the margins are zero bits, every own frame is overwritten, the surroundings untouched.
Both kernels select (csrc/tcm.hip: ``ok ? .. : 0``) or address zeros (csrc/tcm2.hip); neither masks by multiplication,
so NaN serves as the sentinel everywhere (no buffer needed the largest finite float instead)."""
import math
import zlib

import numpy as np
import torch

from conftest import pkg, rel_l2
from helpers import tcm_refs as R

FM = 8                     # floats of NaN in front of and behind a float tensor
HM = 64                    # int16 of NaN pattern in front of and behind an hs tensor (128 bytes: the base stays 16-byte aligned)
NAN16 = 0x7FC0             # NaN as bf16 and as fp16
HS_PAD = 64

SHAPES = [(1, 1), (1, 32), (20, 32), (31, 1), (32, 1), (33, 1), (64, 32), (77, 3), (77, 31), (77, 16), (161, 1), (161, 2), (161, 32)]
FRAMES = {"T_40": lambda T: (T, 40), "0_1": lambda T: (0, 1), "clamped": lambda T: (T + 5, -3), "64_41_T": lambda T: (64, 41, T)}

DEFAULTS = dict(kernel="tcm", np=0, mode=0, T=77, dil=3, B=1, params="nominal", xscale=1.0, chained=True, alias=False,
                frames=None, np_field=None, dils=None)


def _c(name, **kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    c = dict(DEFAULTS, id=name, **kw)
    if c["frames"]:
        c["B"] = len(FRAMES[c["frames"]](c["T"]))
    return c


def _sweep(prefix, **kw):
    """Every shape of SHAPES, chained, parameters and batch size alternating."""
    return [_c("%s_T%d_d%d" % (prefix, T, dil), T=T, dil=dil, B=(1, 3)[i % 2], params=("nominal", "hostile")[i % 2], **kw)
            for i, (T, dil) in enumerate(SHAPES)]


def _forms(prefix, **kw):
    out = [_c(prefix + "_last_T77_d3", params="hostile", chained=False, B=3, **kw),
           _c(prefix + "_alias_T33_d1", T=33, dil=1, alias=True, B=3, **kw),
           _c(prefix + "_alias_T161_d32", T=161, dil=32, alias=True, params="hostile", **kw),
           _c(prefix + "_saturated_T77_d16", dil=16, params="saturated", B=3, **kw),
           _c(prefix + "_saturated_T33_d1", T=33, dil=1, params="saturated", **kw),
           _c(prefix + "_x2e-6_T77_d3", xscale=2.0 ** -6, **kw),
           _c(prefix + "_x8_T77_d3", xscale=8.0, B=3, **kw)]
    for i, name in enumerate(FRAMES):
        out.append(_c("%s_frames_%s_T77_d3" % (prefix, name), frames=name, params=("hostile", "nominal")[i % 2], **kw))
    out.append(_c(prefix + "_frames_64_41_T_T161_d32", T=161, dil=32, frames="64_41_T", **kw))
    out.append(_c(prefix + "_frames_0_1_T20_d32", T=20, dil=32, frames="0_1", params="hostile", **kw))
    return out


TCM = _sweep("tcm") + _forms("tcm")


def _tcm2(npl):
    kw = dict(kernel="tcm2", np=npl)
    p = "tcm2np%d" % npl
    out = _sweep(p, **kw) + _forms(p, **kw)
    out += [_c("%s_mode1_T%d" % (p, T), mode=1, T=T, dil=1, B=B, params=par, **kw)
            for T, B, par in ((1, 3, "hostile"), (33, 1, "nominal"), (77, 3, "hostile"), (161, 1, "nominal"))]
    out.append(_c(p + "_mode1_frames_T_40_T77", mode=1, dil=1, frames="T_40", params="hostile", **kw))
    if npl == 3:
        out.append(_c(p + "_np0_T77_d3", B=3, params="hostile", np_field=0, **kw))
        out.append(_c(p + "_np0_mode1_T33", mode=1, T=33, dil=1, np_field=0, **kw))
    if npl == 2:
        out.append(_c(p + "_wscale_T77_d3", B=3, params="wscale", **kw))
        out.append(_c(p + "_wscale_T161_d32", T=161, dil=32, params="wscale", **kw))
    return out


TCM2 = {npl: _tcm2(npl) for npl in (1, 2, 3)}
STACK_DILS = (1, 32, 2)
TCM2S = {npl: [_c("tcm2snp%d_T161_B2" % npl, kernel="tcm2s", np=npl, T=161, B=2, dils=STACK_DILS, params="hostile"),
               _c("tcm2snp%d_T33" % npl, kernel="tcm2s", np=npl, T=33, B=3, dils=STACK_DILS),
               _c("tcm2snp%d_frames_64_41_T_T161" % npl, kernel="tcm2s", np=npl, T=161, dils=STACK_DILS, frames="64_41_T",
                  params="hostile")] for npl in (1, 2, 3)}
ALL = TCM + [c for npl in (1, 2, 3) for c in TCM2[npl] + TCM2S[npl]]


def by_id(cases):
    return [c["id"] for c in cases]


def find(name):
    return next(c for c in ALL if c["id"] == name)


# ---- natural parameters -------------------------------------------------------------------------------------------------
HOSTILE_SLOPES = (-0.5, 0.0, 1.0, 1.7)


def params(kind, g, slopes=None):
    """One block's natural parameters (tcm_refs.KEYS), float32 numpy, per-channel values random and distinct.
    slopes: (main, mask, conv2) for the hostile set."""
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).numpy()          # noqa: E731
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32).numpy()            # noqa: E731
    p = dict(W1=randn(64, 256) / 16.0, Wm=randn(64, 64, 5) / math.sqrt(320.0), Wk=randn(64, 64, 5) / math.sqrt(320.0),
             W2=randn(256, 64) / 8.0)
    hostile = kind == "hostile"
    amp = 1.0 if hostile else 0.1
    for key, n in (("b1", 64), ("bm", 64), ("bk", 64), ("b2", 256), ("t_main", 64), ("t_mask", 64), ("t2", 64)):
        p[key] = (amp * randn(n)).astype(np.float32)
    for i, key in enumerate(("s_main", "s_mask", "s2")):
        s = 0.65 + 1.05 * rand(64)
        if hostile:                                   # mixed sign, two channels exactly zero
            s = s * np.where(rand(64) < 0.5, -1.0, 1.0).astype(np.float32)
            s[[(7 + 11 * i) % 64, (40 + 5 * i) % 64]] = 0.0
        p[key] = s.astype(np.float32)
    for i, key in enumerate(("a_main", "a_mask", "a2")):
        p[key] = float(np.float32(slopes[i] if hostile else 0.1 + 0.3 * float(rand(1)[0])))
    if kind == "saturated":                           # beyond the fp32 range of exp: the gate is main, respectively 0
        p["bk"][0::3] = 90.0
        p["bk"][1::3] = -90.0
    return p


def block_params(case, n):
    """n + 1 parameter sets: the n blocks of the case and the block whose conv1 is chained onto the last one."""
    g = torch.Generator().manual_seed(zlib.crc32(("par:" + case["id"]).encode()))
    kind = case["params"]
    perm = [HOSTILE_SLOPES[i] for i in torch.randperm(4, generator=g).tolist()]
    out = []
    for i in range(n + 1):
        # main, mask, conv2 pairwise different, and so are the next block's two and this block's conv2
        r = perm[(3 * i) % 4:] + perm[:(3 * i) % 4]
        p = params("nominal" if kind == "wscale" else kind, g, slopes=(r[0], r[1], r[2]))
        if kind == "wscale":                          # the three weight groups of a block at 2^-10, 1, 2^6 - with sane values
            p["Wm"], p["Wk"], p["bm"] = p["Wm"] * 2.0 ** -10, p["Wk"] * 2.0 ** -10, p["bm"] * 2.0 ** -10
            p["s2"] = p["s2"] * 2.0 ** 10
            p["W1"] = p["W1"] * 2.0 ** 6
            p["s_main"], p["s_mask"] = p["s_main"] * 2.0 ** -6, p["s_mask"] * 2.0 ** -6
        out.append({k: (np.ascontiguousarray(v, np.float32) if isinstance(v, np.ndarray) else v) for k, v in p.items()})
    return out


def natural_from_sd(sd, prefix):
    """The natural parameters of one Residual of a DiffUNet1 state dict (keys ``prefix``.conv1 / .mainbranch / .maskbranch /
    .conv2: PReLU, BatchNorm1d, Conv1d in that order)."""
    def a(k):
        v = sd[prefix + "." + k]
        return v.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(v) else np.asarray(v, np.float64)

    def bn(q):
        scale = a(q + ".weight") / np.sqrt(a(q + ".running_var") + 1e-5)
        return scale.astype(np.float32), (a(q + ".bias") - a(q + ".running_mean") * scale).astype(np.float32)

    p = dict(W1=a("conv1.weight")[:, :, 0], b1=a("conv1.bias"), Wm=a("mainbranch.2.weight"), bm=a("mainbranch.2.bias"),
             Wk=a("maskbranch.2.weight"), bk=a("maskbranch.2.bias"), W2=a("conv2.2.weight")[:, :, 0], b2=a("conv2.2.bias"),
             a_main=float(a("mainbranch.0.weight")[0]), a_mask=float(a("maskbranch.0.weight")[0]), a2=float(a("conv2.0.weight")[0]))
    p["s_main"], p["t_main"] = bn("mainbranch.1")
    p["s_mask"], p["t_mask"] = bn("maskbranch.1")
    p["s2"], p["t2"] = bn("conv2.1")
    return p


# ---- descriptor fields from natural parameters (packing.tcm_fields / tcm2_fields, recorded by nets.EpsNetPlan._residual_fused / _residual_split) ----
def _kmat(W):
    """[64 out, 64 in, 5] -> [320, 64]: row = tap * 64 + input channel."""
    return np.concatenate([W[:, :, k].T for k in range(5)], axis=0)


def tcm_fields(p, p_next):
    """Operands (numpy) and scalars of a pdse_tcm_desc."""
    P = pkg("packing")
    f = dict(wbr=P.pack_tcm_branch(_kmat(p["Wm"]), _kmat(p["Wk"])), bmain=p["bm"], bmask=p["bk"],
             xf=np.stack([np.stack([p["s_main"], p["t_main"]], 1), np.stack([p["s_mask"], p["t_mask"]], 1)], 0).astype(np.float32),
             wc2=P.pack_tcm_conv2(p["W2"].T), bc2=p["b2"], xf2=np.stack([p["s2"], p["t2"]], 1).astype(np.float32),
             slope_main=float(p["a_main"]), slope_mask=float(p["a_mask"]), slope2=float(p["a2"]))
    if p_next is not None:
        f["wn1"], f["bn1"] = P.pack_tcm_next(p_next["W1"]), p_next["b1"]
    return f


def tcm2_fields(p, p_next, npl, mode=0):
    """Operands (numpy; uint16 for the packed weights) and scalars of a pdse_tcm2_desc."""
    P = pkg("packing")
    par = np.zeros(832, np.float32)
    f = dict(slope2=0.0, slope_main_next=0.0, slope_mask_next=0.0)
    qof = (lambda *m: P.f16_wexp(*m)) if npl == 2 else (lambda *m: 0)
    qA = q2 = qN = 0
    if mode == 0:
        kmain, kmask = _kmat(p["Wm"]), _kmat(p["Wk"])
        par[:256] = np.stack([p["bm"], p["bk"], p["s2"], p["t2"]], 1).reshape(-1)
        par[256:512] = p["b2"]
        k2 = p["W2"].T
        qA, q2 = qof(kmain, kmask), qof(k2)
        f.update(wbr=P.pack_tcm2_branch(kmain, kmask, npl, qA), wc2=P.pack_tcm2_conv2(k2, npl, q2), slope2=float(p["a2"]))
    if p_next is not None:
        par[512:576] = p_next["b1"]
        par[576:] = np.stack([p_next["s_main"], p_next["t_main"], p_next["s_mask"], p_next["t_mask"]], 1).reshape(-1)
        qN = qof(p_next["W1"])
        f.update(wn1=P.pack_bglu_chain(p_next["W1"], npl, qN), slope_main_next=float(p_next["a_main"]),
                 slope_mask_next=float(p_next["a_mask"]))
    f["par"], f["qexp"] = par, (qA, q2, qN)
    return f


# ---- buffers --------------------------------------------------------------------------------------------------------------
class Built:
    pass


def _fbuf(data, n, device):
    big = torch.full((n + 2 * FM,), math.nan)
    if data is not None:
        big[FM:FM + n] = torch.as_tensor(data, dtype=torch.float32).reshape(-1)
    return big.to(device)


def _hsbuf(hs, shape, device):
    """hs: uint16 array of ``shape`` (margins zero), or None: zero margins, own frames holding the NaN pattern."""
    n = int(np.prod(shape))
    if hs is None:
        hs = np.zeros(shape, np.uint16)
        hs[..., HS_PAD:shape[-2] - HS_PAD, :] = NAN16
    big = np.full(n + 2 * HM, NAN16, np.uint16)
    big[HM:HM + n] = np.asarray(hs, np.uint16).reshape(-1)
    return torch.from_numpy(big.view(np.int16)).to(device)


def fptr(t):
    return t.data_ptr() + 4 * FM


def hptr(t):
    return t.data_ptr() + 2 * HM


def build(case, device):
    """The case as one descriptor on ``device``: Built with desc, the buffers, keep (every tensor a pointer names) and
    ref(dtype, rnd=False) -> what tcm_refs says the launch computes (for the stack: a list, one dict per block)."""
    L, P = pkg("_lib"), pkg("packing")
    c = case
    B, T, npl, kern = c["B"], c["T"], c["np"], c["kernel"]
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    dils = list(c["dils"]) if kern == "tcm2s" else [c["dil"]]
    nblk = len(dils)
    ps = block_params(c, nblk)
    frames = list(FRAMES[c["frames"]](T)) if c["frames"] else None
    out = Built()
    keep = out.keep = []

    def up(a, dtype=np.float32):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)
        keep.append(t)
        return t.data_ptr()

    up16 = lambda a: up(np.asarray(a).view(np.int16), np.int16)                          # noqa: E731
    x = (torch.randn(B, 256, T, generator=g, dtype=torch.float32) * c["xscale"])
    fr_t = None
    if frames is not None:
        fr_t = torch.tensor(frames, dtype=torch.int32).to(device)
        keep.append(fr_t)
    out.case, out.frames, out.x, out.params = c, frames, x, ps
    out.xbuf = _fbuf(x, B * 256 * T, device)
    out.xobuf = out.xbuf if c["alias"] else _fbuf(None, B * 256 * T, device)
    keep += [out.xbuf, out.xobuf]
    # the block's input: h = conv1(x) as the previous launch left it (fp32)
    h = R.conv1(x, ps[0]).to(torch.float32)
    out.h = h
    if kern == "tcm":
        d = L.TcmDesc()
        fields = tcm_fields(ps[0], ps[1] if c["chained"] else None)
        for k, v in fields.items():
            setattr(d, k, up(v) if isinstance(v, np.ndarray) else v)
        out.hbuf = _fbuf(h, B * 64 * T, device)
        out.hobuf = _fbuf(None, B * 64 * T, device)
        keep += [out.hbuf, out.hobuf]
        d.x, d.h, d.x_out = fptr(out.xbuf), fptr(out.hbuf), fptr(out.xobuf)
        if c["chained"]:
            d.h_out = fptr(out.hobuf)
        d.dil, d.B, d.T = c["dil"], B, T
        d.frames = fr_t.data_ptr() if fr_t is not None else 0
        out.desc = d
        out.ref = lambda dtype, rnd=False: R.block(x, ps[0], c["dil"], ps[1] if c["chained"] else None, dtype, frames, h=h)
        return out

    shape = P.tcm2_hs_shape(B, T, npl)
    # the transformed h as its planes carry it (np 3: exactly the fp32 value; np 2 / 1: what the split keeps), zero behind an utterance
    vm, vk = R.transforms(h, ps[0], torch.float32, frames)
    hs_in = P.tcm2_split_h(vm.numpy(), vk.numpy(), npl)
    v_in = tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in P.tcm2_join_h(hs_in, B, T))
    out.v_in = v_in
    out.hsbuf = [_hsbuf(hs_in if c["mode"] == 0 else None, shape, device), _hsbuf(None, shape, device)]
    keep += out.hsbuf

    def one(i, p, p_next, mode, xin, xout, hin, hout):
        d = L.Tcm2Desc()
        for k, v in tcm2_fields(p, p_next, npl, mode).items():
            setattr(d, k, (up16(v) if v.dtype == np.uint16 else up(v)) if isinstance(v, np.ndarray) else v)
        d.x = fptr(xin)
        if mode == 0:
            d.x_out, d.hs = fptr(xout), hptr(hin)
        if p_next is not None:
            d.hs_out = hptr(hout)
        d.dil, d.B, d.T, d.mode = dils[i], B, T, mode
        d.np = npl if c["np_field"] is None else c["np_field"]
        d.frames = fr_t.data_ptr() if fr_t is not None else 0
        return d

    if kern == "tcm2":
        if c["mode"] == 1:
            out.desc = one(0, None, ps[0], 1, out.xbuf, None, None, out.hsbuf[0])
            out.hs_out = out.hsbuf[0]
            out.ref = lambda dtype, rnd=False: R.head(x, ps[0], dtype, frames, rnd)
        else:
            nxt = ps[1] if c["chained"] else None
            out.desc = one(0, ps[0], nxt, 0, out.xbuf, out.xobuf, out.hsbuf[0], out.hsbuf[1])
            out.hs_out = out.hsbuf[1]
            out.ref = lambda dtype, rnd=False: R.block(x, ps[0], c["dil"], nxt, dtype, frames, rnd, v=v_in)
        return out

    # the stack: x ping-pongs between two buffers, hs between its two; every block chained, the last one onto ps[n]
    d = L.Tcm2sDesc()
    xb, hb = [out.xbuf, out.xobuf], out.hsbuf
    for i in range(nblk):
        d.blk[i] = one(i, ps[i], ps[i + 1], 0, xb[i % 2], xb[(i + 1) % 2], hb[i % 2], hb[(i + 1) % 2])
    d.n = nblk
    out.flags = torch.full((B * ((T + 31) // 32),), -1, dtype=torch.int32).to(device)     # zeroed by the launch
    out.status = torch.zeros(4, dtype=torch.int32).to(device)
    keep += [out.flags, out.status]
    d.flags, d.status = out.flags.data_ptr(), out.status.data_ptr()
    out.desc = d
    out.x_last, out.x_prev, out.hs_out = xb[nblk % 2], xb[(nblk - 1) % 2], hb[nblk % 2]

    def compose(dtype, rnd=False):
        res, xi, v = [], x, v_in
        for i in range(nblk):
            r = R.block(xi, ps[i], dils[i], ps[i + 1], dtype, frames, rnd, v=v)
            res.append(r)
            xi, v = r["x_out"], (r["vm_next"], r["vk_next"])
        return res

    out.ref = compose
    return out


# ---- reading the results back ------------------------------------------------------------------------------------------------
def read_f(buf, shape):
    """The tensor inside a float allocation: every element finite, the margins still NaN bit for bit."""
    flat = buf.detach().cpu()
    n = int(np.prod(shape))
    nanbits = torch.full((1,), math.nan).view(torch.int32)
    edge = torch.cat([flat[:FM], flat[FM + n:]]).view(torch.int32)
    assert bool((edge == nanbits).all()), "stored outside the tensor"
    got = flat[FM:FM + n]
    assert bool(torch.isfinite(got).all()), "%d elements not finite (not stored, or poisoned from a margin)" % int((~torch.isfinite(got)).sum())
    return got.reshape(shape).clone()


def untouched_f(buf):
    flat = buf.detach().cpu().view(torch.int32)
    return bool((flat == torch.full((1,), math.nan).view(torch.int32)).all())


def read_hs(buf, B, T, npl):
    """(v_main, v_mask) float32 [B, 64, T] of an hs allocation: the surroundings still hold the NaN pattern, the 64-frame
    margins are zero bits (tcm2_join_h asserts it), every own frame was overwritten (a plane left as it was makes a NaN)."""
    P = pkg("packing")
    raw = buf.detach().cpu().numpy().view(np.uint16)
    n = int(np.prod(P.tcm2_hs_shape(B, T, npl)))
    assert (raw[:HM] == NAN16).all() and (raw[HM + n:] == NAN16).all(), "stored outside the hs tensor"
    vm, vk = P.tcm2_join_h(raw[HM:HM + n], B, T)
    assert np.isfinite(vm).all() and np.isfinite(vk).all(), "own frames of hs_out not overwritten"
    return torch.from_numpy(vm), torch.from_numpy(vk)


def untouched_hs(buf, shape):
    raw = buf.detach().cpu().numpy().view(np.uint16)
    n = int(np.prod(shape))
    inner = raw[HM:HM + n].reshape(shape)
    return bool((raw[:HM] == NAN16).all() and (raw[HM + n:] == NAN16).all() and (inner[..., HS_PAD:shape[-2] - HS_PAD, :] == NAN16).all()
                and not inner[..., :HS_PAD, :].any() and not inner[..., shape[-2] - HS_PAD:, :].any())


def zero_tail(v, frames):
    """hs_out is zero bits from frames[b] to T (tcm2_join_h of zero planes: +0.0)."""
    T = v.shape[-1]
    return all(not v[b, :, f:].numpy().view(np.uint32).any() for b, f in enumerate(R.clamp_frames(frames, T)))


def own(t, frames):
    """The utterances' own frames of [B, C, T] as one flat float64 array (frames None: everything)."""
    t = torch.as_tensor(t)
    if frames is None:
        return t.double().reshape(-1).numpy()
    fr = R.clamp_frames(frames, t.shape[-1])
    return torch.cat([t[b, :, :f].double().reshape(-1) for b, f in enumerate(fr)]).numpy()


# ---- tolerances -------------------------------------------------------------------------------------------------------------
def check_fp32(what, got, ref64, ref32, frames):
    """The project's rule, unchanged: with e32 the error of the same statement evaluated in fp32 on the CPU,
    rel_l2(result, float64) <= max(4 * e32, 2e-6), over the utterances' own frames."""
    got, ref64, ref32 = own(got, frames), own(ref64, frames), own(ref32, frames)
    if ref64.size == 0:
        return 0.0, 0.0
    e32 = rel_l2(ref32, ref64)                                                           # fp32 on the CPU against float64
    err = rel_l2(got, ref64)                                                             # bound: max(4 * e32, 2e-6)
    bound = max(4 * e32, 2e-6)
    print("%s: result %.3e  fp32 cpu %.3e  bound %.3e  result/e32 %.2f" % (what, err, e32, bound, err / e32 if e32 else math.inf))
    assert np.isfinite(err) and err <= bound, (what, err, e32, bound)
    return err, e32


def check_bf16(what, got, rnd64, rnd32, plain64, frames, div=16):
    """np = 1: rel_l2(result, bf16-rounding float64 reference) <= max(4 * e32, e_b / 16), e32 between the fp32 and the float64
    rounding references, e_b = rel_l2(rounding reference, unrounded reference), both float64.  div: the divisor where it is
    not this file's 16 (tests/test_gpu_bglu_ops.py states its own)."""
    got, rnd64, rnd32, plain64 = own(got, frames), own(rnd64, frames), own(rnd32, frames), own(plain64, frames)
    if rnd64.size == 0:
        return 0.0, 0.0, 0.0
    e_b = rel_l2(rnd64, plain64)                                                         # e_b: what the roundings of np = 1 cost
    e32 = rel_l2(rnd32, rnd64)                                                           # fp32 against float64, both rounding (flips included)
    err = rel_l2(got, rnd64)                                                             # bound: max(4 * e32, e_b / 16)
    bound = max(4 * e32, e_b / div)
    print("%s: result %.3e  e_b %.3e  e_b/%d %.3e  fp32 cpu %.3e  bound %.3e  result/(e_b/%d) %.2f" % (
        what, err, e_b, div, e_b / div, e32, bound, div, div * err / e_b if e_b else math.inf))
    assert np.isfinite(err) and err <= bound, (what, err, e_b, e32, bound)
    return err, e_b, e32


def check_hs_bf16(what, got, x_in, p_next, frames):
    """np = 1, hs_out element by element against the unrounded float64 transforms of the chained conv1 on the kernel's own
    input ``x_in`` (rounded to bf16 as the kernel rounds it, bf16 weights):
        |got - ref| <= 2^-8 |ref| + max(4 * e32, 2e-6) * ||ref||_2
    one round-to-nearest is 2^-9 |ref|, the factor two covers a value that fp32 noise carried across a tie; the second term is
    the absolute allowance the fp32 rule gives the tensor (e32: the same statement in fp32 against float64)."""
    r64 = R.head(x_in, p_next, torch.float64, None, True)
    r32 = R.head(x_in, p_next, torch.float32, None, True)
    worst = 0.0
    for br, g_ in zip(("vm_next", "vk_next"), got):
        # unrounded transforms: undo nothing, recompute without the last rounding
        ref = R.transforms(r64["h_out"], p_next, torch.float64)[0 if br == "vm_next" else 1]
        ref32 = R.transforms(r32["h_out"], p_next, torch.float32)[0 if br == "vm_next" else 1]
        a, b, c32 = own(g_, frames), own(ref, frames), own(ref32, frames)
        if b.size == 0:
            continue
        worst = max(worst, check_elems_bf16((what, br), a, b, c32))
    print("%s: hs_out worst |diff| / (2^-8 |ref| + allowance) %.3f" % (what, worst))
    return worst


def check_elems_bf16(what, a, b, c32):
    """The element rule of check_hs_bf16 on flat arrays: a the bf16 values a kernel stored, b the unrounded float64 reference, c32
    the same statement in fp32.  -> the worst |a - b| / (2^-8 |b| + allowance)."""
    e32 = rel_l2(c32, b)                                                                 # fp32 on the CPU against float64 (unrounded)
    allow = max(4 * e32, 2e-6) * float(np.linalg.norm(b))
    excess = np.abs(a - b) - (2.0 ** -8 * np.abs(b) + allow)
    worst = float(np.max(np.abs(a - b) / (2.0 ** -8 * np.abs(b) + allow)))
    assert (excess <= 0).all(), (what, int((excess > 0).sum()), float(excess.max()))
    return worst


def tensors(built):
    """Every CPU tensor the descriptor may point at (tests/emu.py resolves raw pointers through these)."""
    return built.keep
