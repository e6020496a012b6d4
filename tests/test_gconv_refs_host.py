"""CPU: (1) the float64 statement of the gather-GEMM convolution (tests/helpers/gconv_refs.py) against torch's own
convolutions in double; (2) the packers (pack_a, pack_a4 / korder1_rows, pack_s3_gemm) at every descriptor shape of
tests/test_gpu_gconv_ops.py - channel counts, tile tails and chunk tails the networks never use - by replaying the
descriptor on tests/emu.py and holding it to the reference under the GPU file's own rule; (3) the routing: each case
lands on the korder it names."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import emu
from conftest import pkg
from helpers import gconv_cases as G
from helpers import gconv_refs as R

TOL = dict(atol=1e-12, rtol=1e-12)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


# ------------------------------------------------------------------ the reference against torch
@pytest.mark.parametrize("stride", [1, 2])
def test_ref_conv2d_causal(stride):
    P = pkg("packing")
    g = _gen(1)
    B, Cin, Cout, T, Fin = 2, 3, 5, 4, 11
    x, w, b = _randn(g, B, Cin, T, Fin), _randn(g, Cout, Cin, 2, 3), _randn(g, Cout)
    want = F.conv2d(F.pad(x, (0, 0, 1, 0)), w, b, stride=(1, stride))                   # causal: one frame of padding on top
    kk, taps = P.conv_taps(2, 3, 1)
    got = R.gconv(x, taps=taps, Wk0=P.conv_kmat(w, kk), bias0=b, Tout=T, Fout=want.shape[-1], sf_in=stride)
    torch.testing.assert_close(got, want, **TOL)


def test_ref_conv_transpose2d_from_phases():
    P = pkg("packing")
    g = _gen(2)
    B, Cin, Cout, T, Fin = 2, 4, 3, 5, 6
    x, w, b = _randn(g, B, Cin, T, Fin), _randn(g, Cin, Cout, 2, 3), _randn(g, Cout)
    want = F.conv_transpose2d(x, w, b, stride=(1, 2))[:, :, :T]                         # [B, Cout, T, 2 Fin + 1], causal crop
    got = torch.empty_like(want)
    for phase in (0, 1):
        kk, taps = P.convT_phase_taps(2, 3, phase)
        n = want[..., phase::2].shape[-1]
        got[..., phase::2] = R.gconv(x, taps=taps, Wk0=P.convT_kmat(w, kk), bias0=b, Tout=T, Fout=n)
    torch.testing.assert_close(got, want, **TOL)


def test_ref_linear_over_bins_cin1():
    g = _gen(3)
    B, T, Fin, Cout = 2, 5, 7, 9
    x, w, b = _randn(g, B, 1, T, Fin), _randn(g, Cout, Fin), _randn(g, Cout)
    want = F.linear(x[:, 0], w, b).permute(0, 2, 1)[..., None]                          # [B, Cout, T, 1]
    got = R.gconv(x, taps=[(0, k) for k in range(Fin)], Wk0=w.T, bias0=b, Tout=T, Fout=1, cin1=True)
    torch.testing.assert_close(got, want, **TOL)


def test_ref_two_sources_are_a_concatenation():
    g = _gen(4)
    x0, x1, w = _randn(g, 1, 2, 3, 5), _randn(g, 1, 4, 3, 5), _randn(g, 7, 6, 1, 3)
    want = F.conv2d(torch.cat([x0, F.elu(x1)], 1), w, padding=(0, 1))
    P = pkg("packing")
    kk, _ = P.conv_taps(1, 3, 0)
    got = R.gconv(x0, x1, taps=G.TAPS["r3"], Wk0=P.conv_kmat(w, kk), act1=R.ACT_ELU, Tout=3, Fout=5)
    torch.testing.assert_close(got, want, **TOL)


@pytest.mark.parametrize("act", ["none", "elu", "prelu", "sigmoid"])
def test_ref_glu_and_activations(act):
    g = _gen(5)
    x, w, b = _randn(g, 2, 4, 3, 5), _randn(g, 12, 4, 1, 1), _randn(g, 12)
    scale, shift, resid = 0.5 + torch.rand(6, generator=g, dtype=torch.float64), _randn(g, 6), _randn(g, 2, 6, 3, 5)
    y = F.glu(F.conv2d(x, w, b), dim=1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    slope = torch.tensor([0.25], dtype=torch.float64)
    want = {"none": lambda v: v + resid, "elu": F.elu, "prelu": lambda v: F.prelu(v, slope), "sigmoid": torch.sigmoid}[act](y)
    wk = w[:, :, 0, 0].T                                                                 # [Cin, 12]
    got = R.gconv(x, taps=[(0, 0)], Wk0=wk[:, :6], Wk1=wk[:, 6:], bias0=b[:6], bias1=b[6:], epi=R.EPI_GLU, post_scale=scale,
                  post_shift=shift, act_out={"none": 0, "prelu": 1, "elu": 2, "sigmoid": 3}[act], act_slope=0.25,
                  resid=resid if act == "none" else None, Tout=3, Fout=5)
    torch.testing.assert_close(got, want, **TOL)


def test_ref_load_transform_spares_the_padding_and_pad_row_is_frame_minus_one():
    g = _gen(6)
    x, w = _randn(g, 2, 2, 4, 5), _randn(g, 3, 2, 3, 3)
    scale, shift, row = 0.5 + torch.rand(2, generator=g, dtype=torch.float64), 1 + _randn(g, 2), _randn(g, 2, 2)
    P = pkg("packing")
    kk, taps = P.conv_taps(3, 3, 2)                                                      # frames t-2, t-1, t
    taps = [(dt, df - 1) for dt, df in taps]
    xf = dict(mode=1, slope0=0.25, scale0=scale, shift0=shift)
    u = F.prelu(x, torch.tensor([0.25], dtype=torch.float64)) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    # frame -1 is the (untransformed) pad row over the in-range bins, frame -2 and the outer bins are zero
    padded = torch.cat([torch.zeros(2, 2, 1, 5, dtype=torch.float64), row[:, :, None, None].expand(2, 2, 1, 5), u], dim=2)
    want = F.conv2d(F.pad(padded, (1, 1)), w)
    got = R.gconv(x, taps=taps, Wk0=P.conv_kmat(w, kk), xf=xf, padrow=row, Tout=4, Fout=5)
    torch.testing.assert_close(got, want, **TOL)


def test_ref_bf16_operands_and_fp32_evaluation():
    g = _gen(7)
    x, wk = _randn(g, 1, 16, 2, 9).float(), (_randn(g, 16, 8) / 4).float()
    bf = lambda t: t.to(torch.bfloat16).double()                                         # noqa: E731
    want = torch.einsum("km,bktf->bmtf", bf(wk), bf(x))
    got = R.gconv(x, taps=[(0, 0)], Wk0=wk, Tout=2, Fout=9, round_operands="bf16")
    torch.testing.assert_close(got, want, **TOL)
    got32 = R.gconv(x, taps=[(0, 0)], Wk0=wk, Tout=2, Fout=9, dtype=torch.float32)
    assert got32.dtype == torch.float32
    ref = R.gconv(x, taps=[(0, 0)], Wk0=wk, Tout=2, Fout=9)
    assert 0 < float((got32.double() - ref).norm() / ref.norm()) < 1e-6


# ------------------------------------------------------------------ the packers at the GPU file's shapes, and the routing
def _replay(case, korder=None, **kw):
    b = G.build(case, "cpu", korder, **kw)
    assert b.desc.korder == (case["korder"] if korder is None else korder), "routed to korder %d" % b.desc.korder
    emu.run_gconv(b.desc, emu.Mem(G.tensors(b)))
    got = G.check_stores(b)
    G.check_norm(got, b.ref(torch.float64), b.ref(torch.float32))
    return b, got


@pytest.mark.parametrize("case", G.GENERIC, ids=G.by_id(G.GENERIC))
def test_generic_cases_on_the_emulator(case):
    _replay(case)


@pytest.mark.parametrize("case", G.K1, ids=G.by_id(G.K1))
def test_pipelined_cases_on_the_emulator(case):
    b, _ = _replay(case)
    rows = pkg("packing").korder1_rows(len(G.TAPS[case["taps"]]), case["C0"], case["C1"],
                                       pkg("packing").V2_CP[(case["epi"], b.desc.ntaps, case["C1"] > 0, case["xf"])])
    assert b.desc.ksteps == len(rows) // 2 and b.desc.ksteps % 4 == 0


def test_pipelined_cases_cover_every_linear_and_glu_row():
    P = pkg("packing")
    want = {k for k in P.V2_CP if k[0] in (G.LIN, G.GLU)}
    got = {(c["epi"], len(G.TAPS[c["taps"]]), c["C1"] > 0, c["xf"]) for c in G.K1}
    assert got == want and len(want) == 10
    for name, epi, taps, two, xf, cp, _ in G.V2_ROWS:
        assert P.V2_CP[(epi, len(G.TAPS[taps]), two, xf)] == cp, name
        full, part = G.V2_WIDTHS[cp]
        assert (full // 2) % cp == 0 and (part // 2) % cp != 0


@pytest.mark.parametrize("case,mt,max_mt", G.K1_WIDE, ids=[w[0]["id"] for w in G.K1_WIDE])
def test_widening_shapes_follow_pick_mt(case, mt, max_mt):
    """The shapes are derived from the rule; this states the rule once more in numbers, so that a change of the threshold
    in csrc/gconv2.hip shows up as a test to update: 2048 waves after widening, one power of two less does not widen."""
    B, P, Cout = case["B"], case["Tout"] * case["Fout"], case["Cout"]
    tiles, mtiles = B * ((P + 31) // 32), (Cout + 31) // 32
    assert G.pick_mt(B, P, Cout, max_mt) == mt
    assert tiles * ((mtiles + mt - 1) // mt) >= 2048
    assert G.pick_mt(B, P // 2, Cout, max_mt) < mt
    grid = ((P + 31) // 32 + 3) // 4, B, (mtiles + mt - 1) // mt
    assert grid[0] * 4 * grid[1] * grid[2] >= 2048
    _replay(case)


@pytest.mark.parametrize("korder", [3, 4, 5])
@pytest.mark.parametrize("case", G.GEMM, ids=G.by_id(G.GEMM))
def test_gemm_cases_on_the_emulator(case, korder):
    _replay(case, korder)


@pytest.mark.parametrize("case", G.GEMM_WSCALE, ids=G.by_id(G.GEMM_WSCALE))
def test_f16x2_weight_exponent_on_the_emulator(case):
    b, _ = _replay(case, 5)
    assert b.desc.wexp == 13 - int(np.floor(np.log2(np.abs(b.w["wk0"]).max())))     # max |w| 2^wexp in [2^13, 2^14)


def test_f16x2_weight_exponents_differ():
    e = [G.build(c, "cpu", 5).desc.wexp for c in G.GEMM_WSCALE]
    assert abs(e[0] - e[1] - 16) <= 1 and all(-40 <= v <= 40 for v in e)      # two draws of weights, scaled 2^16 apart


@pytest.mark.parametrize("korder", [3, 4, 5])
def test_chained_pair_on_the_emulator(korder):
    ca, cb = G.CHAIN
    a, _ = _replay(ca, korder)
    strides, off = a.layout
    b = G.build(cb, "cpu", korder, src=(a.buf, G.MARGIN + off, (strides[0], strides[1], strides[3], strides[4])),
                src_ref=None)
    assert b.desc.korder == korder and b.desc.in0.blk == 8
    emu.run_gconv(b.desc, emu.Mem(G.tensors(b) + G.tensors(a)))
    G.check_norm(G.check_stores(b), b.ref(torch.float64, a.ref(torch.float64)), b.ref(torch.float32, a.ref(torch.float32)))
