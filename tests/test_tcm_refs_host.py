"""CPU: (1) the statement of the TCM residual block in tests/helpers/tcm_refs.py against a Residual assembled here from
torch.nn's Conv1d / PReLU / BatchNorm1d (eval) in double; (2) every case of tests/helpers/tcm_cases.py - the descriptors
tests/test_gpu_tcm_ops.py launches - replayed on tests/emu.py (run_tcm, run_tcm2, run_tcm2s) and held to the float64
reference at 1e-6, which pins packers and descriptor construction without a GPU, together with the f16x2 window of
every np = 2 case; (3) the case helper's descriptor fields against the descriptors nets.EpsNetPlan records for a
synthetic DiffUNet1 - on EpsNetPlan itself (_residual_fused, _residual_split at np 1 / 2 / 3, both modes, which record what
packing.tcm_fields / packing.tcm2_fields pack), byte for byte."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import emu
from conftest import pkg, rel_l2, tcm2_blocks
from helpers import tcm_cases as G
from helpers import tcm_refs as R

TOL = dict(atol=1e-12, rtol=1e-12)


# ------------------------------------------------------------------ the reference against torch
class TorchResidual(nn.Module):
    """conv1 (1x1, 256 -> 64); two branches PReLU - BatchNorm1d - Conv1d(k = 5, dilation d, padding 2 d), the mask one
    through a sigmoid; their product through PReLU - BatchNorm1d - Conv1d (1x1, 64 -> 256); plus the input."""

    def __init__(self, dil):
        super().__init__()
        branch = lambda: nn.Sequential(nn.PReLU(), nn.BatchNorm1d(64), nn.Conv1d(64, 64, 5, dilation=dil, padding=2 * dil))   # noqa: E731
        self.conv1 = nn.Conv1d(256, 64, 1)
        self.main, self.mask = branch(), branch()
        self.conv2 = nn.Sequential(nn.PReLU(), nn.BatchNorm1d(64), nn.Conv1d(64, 256, 1))

    def forward(self, x):
        h = self.conv1(x)
        return self.conv2(self.main(h) * torch.sigmoid(self.mask(h))) + x


def _random_module(dil, seed, negative_bn):
    g = torch.Generator().manual_seed(seed)
    m = TorchResidual(dil).double().eval()
    with torch.no_grad():
        for name, t in list(m.named_parameters()) + list(m.named_buffers()):
            if name.endswith("num_batches_tracked"):
                continue
            if name.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g, dtype=torch.float64))
            elif t.shape == (1,):                                  # PReLU slope
                t.copy_(torch.rand(1, generator=g, dtype=torch.float64) * 2.0 - 0.7)
            else:
                t.copy_(torch.randn(t.shape, generator=g, dtype=torch.float64) * (0.2 if t.dim() > 1 else 1.0))
        if not negative_bn:
            for seq in (m.main, m.mask, m.conv2):
                seq[1].weight.abs_()
    return m


def _natural(m):
    def bn(b):
        s = b.weight / torch.sqrt(b.running_var + b.eps)
        return s.detach(), (b.bias - b.running_mean * s).detach()

    p = dict(W1=m.conv1.weight[:, :, 0].detach(), b1=m.conv1.bias.detach(), Wm=m.main[2].weight.detach(), bm=m.main[2].bias.detach(),
             Wk=m.mask[2].weight.detach(), bk=m.mask[2].bias.detach(), W2=m.conv2[2].weight[:, :, 0].detach(), b2=m.conv2[2].bias.detach(),
             a_main=float(m.main[0].weight.detach()), a_mask=float(m.mask[0].weight.detach()), a2=float(m.conv2[0].weight.detach()))
    p["s_main"], p["t_main"] = bn(m.main[1])
    p["s_mask"], p["t_mask"] = bn(m.mask[1])
    p["s2"], p["t2"] = bn(m.conv2[1])
    return p


@pytest.mark.parametrize("dil,T,B,negative_bn", [(1, 9, 2, False), (3, 20, 1, True), (32, 70, 2, True), (32, 40, 1, False), (3, 5, 3, True),
                                                 (1, 1, 1, True)])
def test_ref_matches_torch_residual(dil, T, B, negative_bn):
    """Dilations 1, 3 and 32, T < 2 dil (40 and 5), T = 1, negative BatchNorm scales; the chained conv1 and the next block's
    transforms against the next module's own first layers."""
    m, nxt = _random_module(dil, 100 + dil + T, negative_bn), _random_module(1, 200 + dil + T, negative_bn)
    if negative_bn:
        assert bool((m.main[1].weight < 0).any()) and bool((m.conv2[1].weight < 0).any())
    x = torch.randn(B, 256, T, generator=torch.Generator().manual_seed(T), dtype=torch.float64)
    p, pn = _natural(m), _natural(nxt)
    with torch.no_grad():
        want = m(x)
        want_h = nxt.conv1(want)
        want_vm, want_vk = nxt.main[1](nxt.main[0](want_h)), nxt.mask[1](nxt.mask[0](want_h))
    got = R.block(x, p, dil, pn)
    torch.testing.assert_close(got["x_out"], want, **TOL)
    torch.testing.assert_close(got["h_out"], want_h, **TOL)
    torch.testing.assert_close(got["vm_next"], want_vm, **TOL)
    torch.testing.assert_close(got["vk_next"], want_vk, **TOL)
    # the entry points the kernels start from say the same
    with torch.no_grad():
        h = m.conv1(x)
    torch.testing.assert_close(R.block(x, p, dil, h=h)["x_out"], want, **TOL)
    torch.testing.assert_close(R.block(x, p, dil, v=R.transforms(h, p))["x_out"], want, **TOL)


def test_ref_frames_is_the_utterance_alone():
    """frames[b]: utterance b as if it were alone with that many frames - over its own frames the truncated tensor's result,
    the next block's transforms zero behind them; values are clamped to 0 .. T."""
    m, nxt = _random_module(3, 7, True), _random_module(1, 8, True)
    p, pn = _natural(m), _natural(nxt)
    T, frames = 23, (23, 9, 0, 30, -2)
    x = torch.randn(5, 256, T, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    got = R.block(x, p, 3, pn, frames=frames)
    assert R.clamp_frames(frames, T) == [23, 9, 0, 23, 0]
    for b, f in enumerate(R.clamp_frames(frames, T)):
        assert not got["vm_next"][b, :, f:].any() and not got["vk_next"][b, :, f:].any()
        if f:
            with torch.no_grad():
                want = m(x[b:b + 1, :, :f])
            torch.testing.assert_close(got["x_out"][b:b + 1, :, :f], want, **TOL)
            alone = R.block(x[b:b + 1, :, :f], p, 3, pn)
            torch.testing.assert_close(got["vk_next"][b:b + 1, :, :f], alone["vk_next"], **TOL)


def test_ref_bf16_rounding_points():
    """bf16() is round-to-nearest-even on 8 significand bits (torch's own bfloat16 conversion), and rnd moves the result by
    about what four roundings of 2^-9 cost - neither nothing nor a different operation."""
    v = torch.randn(4096, generator=torch.Generator().manual_seed(1), dtype=torch.float32) * 37.0
    assert torch.equal(R.bf16(v), v.to(torch.bfloat16).to(torch.float32))
    assert torch.equal(R.bf16(v.double()), v.to(torch.bfloat16).double())
    tie = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8)], dtype=torch.float64)
    assert R.bf16(tie).tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0]
    b = G.build(G.find("tcm2np1_T77_d3"), "cpu")
    plain, rnd = b.ref(torch.float64), b.ref(torch.float64, True)
    e = rel_l2(rnd["x_out"], plain["x_out"])
    assert 2.0 ** -12 < e < 2.0 ** -6, e
    assert torch.equal(rnd["vm_next"], R.bf16(rnd["vm_next"])) and not torch.equal(plain["vm_next"], R.bf16(plain["vm_next"]))


# ------------------------------------------------------------------ the case table on the emulator
def _replay(case):
    b = G.build(case, "cpu")
    emu.RUNNERS[type(b.desc)](b.desc, emu.Mem(G.tensors(b)))
    return b


def _close(got, want, frames, what):
    a, w = G.own(got, frames), G.own(want, frames)
    if w.size:
        e = rel_l2(a, w)
        assert e <= 1e-6, (what, e)


def _close_hs(case, got, want, frames, what):
    """hs_out.  np 2 / 3: 1e-6 like everything else.  np 1: the emulator rounds the transforms it evaluated in fp32 arithmetic
    (emu.run_tcm2: vm, vk), the reference the float64 value - a value within fp32 noise (2^-23) of a rounding tie (spacing
    2^-8) lands one bf16 ulp away, about one element in 2^14, and ONE such element is 2e-6 of a small tensor.  So there:
    bit-equal to the reference's rounding but for at most one element in 1000, those within one bf16 ulp (2^-7 relative; plus
    1e-6 of the largest value, for a transform that cancels to next to nothing)."""
    if case["np"] != 1:
        return _close(got, want, frames, what)
    a, w = G.own(got, frames), G.own(want, frames)
    if w.size:
        off = a != w
        assert off.sum() <= 1e-3 * w.size and (np.abs(a - w)[off] <= 2.0 ** -7 * np.abs(w[off]) + 1e-6 * np.abs(w).max()).all(), (what, int(off.sum()), w.size)


def _window(case, *tensors):
    """np = 2: every hs value inside the f16x2 window, |value| * 2^PDSE_F16_ACT_EXP < 4094 (include/pdse.h)."""
    if case["np"] == 2:
        P = pkg("packing")
        for t in tensors:
            assert float(torch.as_tensor(t).abs().max()) * 2.0 ** P.F16_ACT_EXP < 4094.0, case["id"]


@pytest.mark.parametrize("case", G.TCM, ids=G.by_id(G.TCM))
def test_emulator_tcm(case):
    b = _replay(case)
    B, T = case["B"], case["T"]
    ref = b.ref(torch.float64)
    _close(G.read_f(b.xobuf, (B, 256, T)), ref["x_out"], b.frames, "x_out")
    if case["chained"]:
        _close(G.read_f(b.hobuf, (B, 64, T)), ref["h_out"], b.frames, "h_out")
    else:
        assert b.desc.h_out is None and G.untouched_f(b.hobuf)


@pytest.mark.parametrize("case", [c for n in (1, 2, 3) for c in G.TCM2[n]], ids=[i for n in (1, 2, 3) for i in G.by_id(G.TCM2[n])])
def test_emulator_tcm2(case):
    b = _replay(case)
    B, T, npl = case["B"], case["T"], case["np"]
    assert b.desc.np == (npl if case["np_field"] is None else 0)
    ref = b.ref(torch.float64, npl == 1)
    _window(case, *b.v_in)
    if case["mode"] == 0:
        _close(G.read_f(b.xobuf, (B, 256, T)), ref["x_out"], b.frames, "x_out")
    else:
        assert G.untouched_f(b.xobuf)
    if case["mode"] == 1 or case["chained"]:
        vm, vk = G.read_hs(b.hs_out, B, T, npl)
        _window(case, ref["vm_next"], ref["vk_next"])
        _close_hs(case, vm, ref["vm_next"], b.frames, "hs_out main")
        _close_hs(case, vk, ref["vk_next"], b.frames, "hs_out mask")
        if b.frames:
            assert G.zero_tail(vm, b.frames) and G.zero_tail(vk, b.frames)
    else:
        assert b.desc.hs_out is None and G.untouched_hs(b.hsbuf[1], pkg("packing").tcm2_hs_shape(B, T, npl))


@pytest.mark.parametrize("case", [c for n in (1, 2, 3) for c in G.TCM2S[n]], ids=[i for n in (1, 2, 3) for i in G.by_id(G.TCM2S[n])])
def test_emulator_tcm2s(case):
    """np 2 / 3: the stack against the composition of the references.  np 1: a rounding the emulator's fp32 transforms carried
    across a tie (see _close_hs) travels on through the later blocks, so there every block is held to the reference on the
    emulator's own inputs, and run_tcm2s to the same bits as that walk."""
    B, T, npl = case["B"], case["T"], case["np"]
    shape = (B, 256, T)
    b = _replay(case)
    vm, vk = G.read_hs(b.hs_out, B, T, npl)
    if b.frames:
        assert G.zero_tail(vm, b.frames) and G.zero_tail(vk, b.frames)
    if npl != 1:
        refs = b.ref(torch.float64)
        _window(case, *b.v_in)
        for r in refs:
            _window(case, r["vm_next"], r["vk_next"])
        _close(G.read_f(b.x_last, shape), refs[-1]["x_out"], b.frames, "x_out of the last block")
        _close(G.read_f(b.x_prev, shape), refs[-2]["x_out"], b.frames, "x_out of the block before")
        _close(vm, refs[-1]["vm_next"], b.frames, "hs_out main")
        _close(vk, refs[-1]["vk_next"], b.frames, "hs_out mask")
        return
    w = G.build(case, "cpu")
    mem, xb, hb = emu.Mem(G.tensors(w)), [w.xbuf, w.xobuf], w.hsbuf
    for i, dil in enumerate(case["dils"]):
        x_in, v_in = G.read_f(xb[i % 2], shape), G.read_hs(hb[i % 2], B, T, npl)
        emu.run_tcm2(w.desc.blk[i], mem)
        r = R.block(x_in, w.params[i], dil, w.params[i + 1], torch.float64, w.frames, True, v=v_in)
        _close(G.read_f(xb[(i + 1) % 2], shape), r["x_out"], w.frames, "x_out of block %d" % i)
        got = G.read_hs(hb[(i + 1) % 2], B, T, npl)
        _close_hs(case, got[0], r["vm_next"], w.frames, "hs_out main of block %d" % i)
        _close_hs(case, got[1], r["vk_next"], w.frames, "hs_out mask of block %d" % i)
    for one, other in ((b.x_last, w.x_last), (b.x_prev, w.x_prev), (b.hs_out, w.hs_out)):
        assert one.numpy().tobytes() == other.numpy().tobytes()


def test_case_table_reaches_what_it_names():
    """Every shape of the table in every sweep; the wscale cases' three exponents pairwise different; hostile slopes from the
    stated set, pairwise different where a swap would otherwise cancel; two BatchNorm scales exactly zero; saturated mask biases."""
    for cases in (G.TCM, G.TCM2[1], G.TCM2[2], G.TCM2[3]):
        assert {(c["T"], c["dil"]) for c in cases if c["mode"] == 0} >= set(G.SHAPES)
    assert max(c["T"] for c in G.ALL) == 161 and {c["B"] for c in G.ALL} >= {1, 3}
    for name in ("tcm2np2_wscale_T77_d3", "tcm2np2_wscale_T161_d32"):
        q = tuple(G.build(G.find(name), "cpu").desc.qexp)
        assert len(set(q)) == 3, q
    p, pn = G.block_params(G.find("tcm2np3_T77_d3"), 1)
    assert len({p["a_main"], p["a_mask"], p["a2"]}) == 3 and pn["a_main"] != pn["a_mask"] and pn["a_main"] != p["a_main"]
    assert {p["a_main"], p["a_mask"], p["a2"], pn["a_main"], pn["a_mask"]} <= {float(np.float32(s)) for s in G.HOSTILE_SLOPES}
    for key in ("s_main", "s_mask", "s2"):
        assert int((p[key] == 0).sum()) == 2 and (p[key] < 0).any() and (p[key] > 0).any()
    sat = G.block_params(G.find("tcm_saturated_T33_d1"), 1)[0]["bk"]
    assert int((sat == 90).sum()) >= 21 and int((sat == -90).sum()) >= 21


# ------------------------------------------------------------------ the descriptor builder against nets.EpsNetPlan
def _bytes(mem, ptr, nbytes, dtype):
    return np.asarray(mem.arr(ptr, nbytes // np.dtype(dtype).itemsize, dtype)).tobytes()


@pytest.mark.parametrize("npl", [0, 1, 2, 3])
def test_descriptor_fields_match_eps_net_plan(weights, npl):
    """npl 0: the fp32 blocks (_residual_fused, 18 descriptors); 1 / 2 / 3: _residual_split, the mode-1 launch and the 18 blocks.
    Packed operands byte for byte, scalar fields equal - on EpsNetPlan itself, built on the CPU context."""
    nets, L = pkg("nets"), pkg("_lib")
    sd = weights("DiffUNet1")
    B, T = 1, 12
    ctx = nets.Ctx("cpu")
    net = nets.EpsNetPlan(ctx, sd, B, T, time_cond=True, nsteps=1, exclusive=True, **(dict(split_bf16=False) if npl == 0 else dict(planes=npl)))
    net.build_time()
    net.build_step(0)
    mem = emu.Mem(ctx.all_tensors())
    names = [("TCMs.%d.residual%d" % (i, j + 1), dil) for i in range(3) for j, dil in enumerate((1, 2, 4, 8, 16, 32))]
    nat = [G.natural_from_sd(sd, p) for p, _ in names]

    def same(d, f, sizes, scalars):
        for key, (n, dtype) in sizes.items():
            if key not in f:
                assert not getattr(d, key), key
                continue
            want = np.ascontiguousarray(f[key], None if f[key].dtype == np.uint16 else np.float32).view(dtype).tobytes()
            assert len(want) == n * np.dtype(dtype).itemsize, key
            assert _bytes(mem, getattr(d, key), len(want), dtype) == want, key
        for key in scalars:
            a, b_ = getattr(d, key), f[key]
            assert (tuple(a) == tuple(b_)) if key == "qexp" else (ctypes.c_float(a).value == ctypes.c_float(b_).value), key

    if npl == 0:
        descs = [d for d, _ in net.descs if isinstance(d, L.TcmDesc)]
        assert len(descs) == 18
        sizes = dict(wbr=(2 * 2 * 20 * 2 * 64 * 4, np.float32), bmain=(64, np.float32), bmask=(64, np.float32), xf=(256, np.float32),
                     wc2=(8 * 8 * 64 * 4, np.float32), bc2=(256, np.float32), xf2=(128, np.float32), wn1=(4 * 2 * 2 * 4 * 64 * 4, np.float32),
                     bn1=(64, np.float32))
        for i, d in enumerate(descs):
            assert d.dil == names[i][1]
            same(d, G.tcm_fields(nat[i], nat[i + 1] if i + 1 < 18 else None), sizes, ("slope_main", "slope_mask", "slope2"))
        return
    descs = tcm2_blocks(net.descs)
    assert len(descs) == 19 and descs[0].mode == 1 and all(d.np == npl for d in descs)
    sizes = dict(wbr=(2 * 2 * 20 * npl * 512, np.int16), wc2=(8 * 4 * npl * 512, np.int16), wn1=(2 * 16 * npl * 512, np.int16),
                 par=(832, np.float32))
    scalars = ("slope2", "slope_main_next", "slope_mask_next", "qexp")
    same(descs[0], G.tcm2_fields(None, nat[0], npl, 1), sizes, scalars)
    for i, d in enumerate(descs[1:]):
        assert d.mode == 0 and d.dil == names[i][1]
        same(d, G.tcm2_fields(nat[i], nat[i + 1] if i + 1 < 18 else None, npl, 0), sizes, scalars)
