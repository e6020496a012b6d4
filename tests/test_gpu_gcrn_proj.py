"""The flat form of the LSTM input projections (pdse_gconv_desc.flat, csrc/gconv4.hip: gconv4_flat_kernel) through the C-ABI,
alone against the float64 statement of the same convolution (tests/helpers/gconv_refs.py via gconv_cases.build), and against
the tiled form of the same descriptor, bit for bit.

Shapes: cin 128, 4 taps ("tp0": two of them one frame back), Cout 2048, Fout 1, at the (B, T) where the flat column index
n = b T + t can go wrong - one column (every tap but one out of range), a 32-column tile that straddles two items (item 1's
frame -1 must read zero, not item 0's last frame), a ragged last tile, the full batch width.  The activations carry an offset of
8 b per item (weights N(0, 1 / K), K = 512: a frame of the wrong item moves an output by about 8 sqrt(128 / 512) = 4, the
tolerance is of the order 1e-6), and every item sits between NaN frames, so a read of the neighbouring allocation poisons the
result.  The output is the channels-innermost layout of the gate buffer (16-byte stores); gconv_cases.check_stores demands that
exactly the addressed elements are written.

Tolerance: the rule of tests/test_gpu_gconv_ops.py unchanged (gconv_cases.check_norm): rel_l2(kernel, float64) <=
max(4 * e32, 2e-6), e32 the error of the fp32 CPU evaluation.  Measured values: profiles/gcrn_proj_margins.txt."""
import math

import pytest
import torch

from conftest import pkg
from helpers import gconv_cases as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1), (2, 33), (3, 21), (32, 5)]
ITEM_OFFSET = 8.0


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    lib = pkg("_lib")
    lib.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return lib


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault fails every later launch of the process: stop instead of piling them on
        pytest.exit("device error after a gconv launch: %s" % e, returncode=3)


def _case(B, T, blk):
    c = dict(G.DEFAULTS, id="proj_b%d_t%d_%s" % (B, T, "blk" if blk else "nchw"), family="gemm", B=B, C0=128, Cout=2048, taps="tp0",
             Tout=T, Fout=1, layout="clast", blk=blk)
    return c


def _source(case):
    """in0 with the per-item offset, in the blocked layout of gconv_cases.build's own sources (a NaN frame and bin around every
    item): (buffer, element offset, strides), reference value."""
    B, C, T = case["B"], case["C0"], case["Tout"]
    g = torch.Generator().manual_seed(G.seed_of(case) ^ 0x5A5A)
    x = torch.randn(B, C, T, 1, generator=g) + ITEM_OFFSET * torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)
    big = torch.full((B, C // 8, T + 2, 3, 8), math.nan)
    big[:, :, 1:-1, 1:-1] = x.view(B, C // 8, 8, T, 1).permute(0, 1, 3, 4, 2)
    st = 3 * 8
    return (big.to(DEV), st + 8, (C // 8 * (T + 2) * st, (T + 2) * st, st, 8)), x


def _build(case, korder):
    if case["blk"]:
        src, x = _source(case)
        b = G.build(case, DEV, korder, src=src, src_ref=x)
        b.keep.append(src[0])
    else:
        b = G.build(case, DEV, korder)      # plain strides: the builder's own N(0, 1) source
    assert b.desc.korder == korder and b.desc.Fout == 1 and b.desc.ntaps * b.desc.in0.C == 512
    return b


def _launch(L, b, flat):
    b.buf.fill_(math.nan)
    b.desc.flat = flat
    L.launch(b.desc)
    _sync()
    return G.check_stores(b)


@pytest.mark.parametrize("korder", [5, 3])
@pytest.mark.parametrize("blk", [True, False], ids=["blk8", "nchw"])
@pytest.mark.parametrize("B,T", SHAPES, ids=["b%d_t%d" % s for s in SHAPES])
def test_flat_projection(L, B, T, blk, korder):
    b = _build(_case(B, T, blk), korder)
    ref64, ref32 = b.ref(torch.float64), b.ref(torch.float32)
    tiled = _launch(L, b, 0)
    print("tiled form: ", end="")
    G.check_norm(tiled, ref64, ref32)
    flat = _launch(L, b, 1)
    print("flat form:  ", end="")
    G.check_norm(flat, ref64, ref32)
    # the K order per output element is that of the tiled form: the same bits
    assert torch.equal(flat.view(torch.int32), tiled.view(torch.int32))


def test_flat_refusals(L):
    """The flat form is one of the korder 3 / 5 LINEAR launches with Fout == 1 and Cout in multiples of 256."""
    b = _build(_case(1, 1, True), 5)
    for name, value in (("Cout", 2048 - 32), ("Fout", 2), ("flat", 2)):
        keep = getattr(b.desc, name)
        b.desc.flat = 1
        setattr(b.desc, name, value)
        with pytest.raises(L.PdseError, match="flat form"):
            L.launch(b.desc)
        setattr(b.desc, name, keep)


def test_plan_switch_is_bit_identical(L):
    """GcrnPlan with flat_proj off and on (B = 2, T = 33: a flat tile straddles the items): the gate buffer gx1 and the prior's
    output, bit for bit."""
    nets, synth = pkg("nets"), pkg("synth")
    sd = synth.make_state_dict("GCRN")
    x = torch.randn(2, 2, 33, 161, generator=torch.Generator().manual_seed(7))
    res = []
    for flat in (False, True):
        cls = type("GcrnPlanAB", (nets.GcrnPlan,), dict(flat_proj=flat))
        net = cls(nets.Ctx(DEV), sd, 2, 33)
        net.build()
        net.finish()
        proj = [d for d, _ in net.descs if isinstance(d, L.GconvDesc) and d.Cout == 2048]
        assert len(proj) == 2 and all(d.flat == int(flat) and d.korder == 5 for d in proj)
        net.x.copy_(x)
        net.plan.run()
        _sync()
        res.append((net.gx.clone(), net.out.clone()))
    assert torch.isfinite(res[1][1]).all()
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32))
    assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))
