"""A decoder stage's phase pair as one launch (csrc/gconv4.hip, gconv4_pair_kernel) against the two launches it replaces.

The even-bin descriptor of a stride-(1,2) transposed GLU convolution (f16x2, korder 5) may name the next operator of the plan
as its odd phase (include/pdse.h: p1mask with w2 == NULL); a plan that runs both in one call runs them as one launch.  Run one by
one (Plan.run_range over a single operator) the same two descriptors are the launches they always were.  The condition is
bit-identity: both forms write into buffers pre-filled with a sentinel, and the WHOLE buffers must be torch.equal - so the one
launch also writes nothing outside the bins the two launches write.  No tolerance anywhere in this file.

Built for stages of at most 32 output channels (one channel tile per workgroup): the 128- and 64-channel stages stay two launches,
GcrnPlan does not mark them (the plan-level test pins it) and a plan refuses a mark on one.  The 16-channel main + gate tile and
the flattened LSTM projections of the same issue are not built; this file has no cases for them."""
import math

import pytest
import torch

from conftest import golden, pkg, rel_l2, seeded
from helpers import gconv_cases as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0


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


def _stage(mark, B, T, Cin, Cout, Fin, extra, blk_out, blk_in=True):
    """One decoder stage as nets.GcrnPlan records it: in0 and in1 (with the re-applied ELU) channel-blocked, or both plain
    [B, C, T, F] (blk_in False: GcrnPlan.block8 off), two
    descriptors (even bins: taps {j, j-1}; odd bins: tap {j}) storing interleaved into one output.  mark: the even-bin descriptor
    names the odd one.  Same seed -> same operands for either setting."""
    nets, P = pkg("nets"), pkg("packing")
    g = torch.Generator().manual_seed(G.seed_of(dict(id="pair_%d_%d_%d_%d_%d" % (T, Cin, Cout, Fin, extra))))
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)      # noqa: E731
    pb = nets.PlanBase(nets.Ctx(DEV))
    pb.gemm_planes = 2
    C0 = Cin // 2
    Fout = 2 * (Fin - 1) + 3 + extra
    x0 = randn(B, C0 // 8, T, Fin, 8).to(DEV)          # the same values under either reading of the layout
    x1 = randn(B, C0 // 8, T, Fin, 8).to(DEV)
    ist = nets.nc8(C0, T, Fin) if blk_in else nets.nchw(C0, T, Fin)
    in0 = pb.src(x0, C0, *ist, blk=8 if blk_in else 0)
    in1 = pb.src(x1, C0, *ist, act=G.ELU, blk=8 if blk_in else 0)
    wt = [randn(Cin, Cout, 1, 3) / math.sqrt(2 * Cin) for _ in range(2)]
    bias = [(0.3 * randn(Cout)).numpy() for _ in range(2)]
    post = ((0.5 + torch.rand(Cout, generator=g)).numpy(), (0.2 * randn(Cout)).numpy())
    if blk_out:
        (osb, osc, olo, ost, osf), ocr = nets.nc8_out(Cout, T, Fout), 8
    else:
        (osb, osc, olo, ost, osf), ocr = nets.nchw_out(Cout, T, Fout), 1
    out = torch.full((B * Cout * T * Fout + 16,), SENTINEL, device=DEV)
    descs = []
    for phase in (0, 1):
        kk, taps = P.convT_phase_taps(1, 3, phase)
        descs.append(pb.gconv(
            in0=in0, in1=in1, Tin=T, Fin=Fin, taps=taps, sf_in=1, Cout=Cout, epi=G.GLU, act=G.ELU,
            W=lambda kk=kk: dict(wk0=P.convT_kmat(wt[0], kk), wk1=P.convT_kmat(wt[1], kk), bias0=bias[0], bias1=bias[1], post=post),
            out=out[8:], out_strides=(osb, osc, olo, ost, 2 * osf), out_off=phase * osf, out_cr=ocr, B=B, Tout=T,
            Fout=(Fout - phase + 1) // 2, label="pair.ph%d" % phase, s3g=True,
            phase1=dict(mask=1, Fout1=Fout // 2) if phase == 0 and mark else None))
    assert all(d.korder == 5 for d in descs) and descs[0].p1mask == (1 if mark else 0) and not descs[0].w2
    pb.finish()
    pb.keepalive = (x0, x1, out)
    return pb, out, Fout


# (Cin, Cout, Fin, extra bin of the k == 2 stage, blocked output, blocked sources): GCRN's conv3_t (d3 is channel-blocked) and
# conv2_t (d2 is not), and conv2_t as a plan with block8 off records it (the kernel's instantiation for plain sources)
STAGES = [(128, 32, 19, 0, True, True), (64, 16, 39, 1, False, True), (64, 16, 39, 1, False, False)]


@pytest.mark.parametrize("T", [5, 33])            # 33: a stage's positions cross 32-frame tiles and workgroups
@pytest.mark.parametrize("Cin,Cout,Fin,extra,blk_out,blk_in", STAGES, ids=["c128_32_f19", "c64_16_f39x", "c64_16_f39x_nchw"])
def test_phase_pair_equals_two_launches(L, T, Cin, Cout, Fin, extra, blk_out, blk_in):
    """Fin = 19 gives Fout = 39: 20 even and 19 odd bins, the ragged last bin; Fin = 39 with the extra bin gives 40 + 40, the
    odd bin of j = 39 reading past the input (zero).  in1 carries the re-applied ELU."""
    B = 2
    one, out1, Fout = _stage(True, B, T, Cin, Cout, Fin, extra, blk_out, blk_in)
    two, out2, _ = _stage(False, B, T, Cin, Cout, Fin, extra, blk_out, blk_in)
    one.plan.run()                       # both operators in one call: one launch
    two.plan.run_range(0, 1)             # the present launches, one by one
    two.plan.run_range(1, 2)
    _sync()
    assert one.plan.time_tag(0)[1] == 1 and two.plan.time_tag(0)[1] == 2      # launches counted by the plan
    _sync()
    written = out2 != SENTINEL
    assert int(written.sum()) == B * Cout * T * Fout and not bool(written[:8].any()) and not bool(written[-8:].any())
    assert torch.equal(out1, out2)
    # the marked descriptors, run one by one, are the two launches too
    out1.fill_(SENTINEL)
    one.plan.run_range(0, 1)
    one.plan.run_range(1, 2)
    _sync()
    assert torch.equal(out1, out2)


def test_a_plan_refuses_what_is_not_a_pair(L):
    """The operator behind a marked descriptor is checked when it is added: an error there, not a silent pair of launches and
    not an error in the middle of a run."""
    nets = pkg("nets")
    pb, out, _ = _stage(True, 2, 5, 64, 16, 39, 1, False)
    d0, d1 = pb.descs[0][0], pb.descs[1][0]
    d1.Tout = 4                                        # not the same frames
    bad = nets.PlanBase(nets.Ctx(DEV))
    bad.plan.add(d0)
    with pytest.raises(L.PdseError, match="odd phase"):
        bad.plan.add(d1)
    with pytest.raises(L.PdseError, match="must be that phase"):
        bad.plan.add(L.EwDesc())                       # another kind of operator
    assert len(bad.plan) == 1
    bad.plan.run()                                     # alone, the marked descriptor is the launch it always was
    _sync()


def test_stages_of_more_than_32_channels_are_refused_as_a_pair(L):
    """GCRN's conv5_t shape (512 -> 128 channels, Fin = 4: Fout = 9, five even and four odd bins).  The one-launch form holds one
    channel tile per workgroup; a mark on a wider stage is refused where the pair enters the plan, and the same two descriptors
    without the mark are the two launches of today."""
    with pytest.raises(L.PdseError, match="Cout <= 32"):
        _stage(True, 2, 5, 512, 128, 4, 0, True)
    pb, out, Fout = _stage(False, 2, 5, 512, 128, 4, 0, True)
    assert Fout == 9 and pb.plan.time_tag(0)[1] == 2
    _sync()
    assert int((out != SENTINEL).sum()) == 2 * 128 * 5 * 9


def test_gcrn_plan_with_and_without_fused_phases(L, weights, monkeypatch):
    """gcrn_small through GcrnPlan with the switch on and off: the prior's output bit for bit, four launches fewer (the 32- and
    16-channel stages of both decoders), and the golden at its tolerance (2e-5, test_gcrn_golden) for the new form."""
    nets = pkg("nets")
    g = golden("gcrn_small")
    x = seeded((2, 2, 20, 161), g["seed_x"]).to(DEV)
    outs, launches = [], []
    for fuse in (True, False):
        monkeypatch.setattr(nets.GcrnPlan, "fuse_phases", fuse)
        net = nets.GcrnPlan(nets.Ctx(DEV), weights("GCRN"), 2, 20)
        net.build()
        net.finish()
        marks = [d for d, _ in net.descs if isinstance(d, L.GconvDesc) and d.korder == 5 and d.p1mask]
        assert len(marks) == (4 if fuse else 0) and all(d.Cout <= 32 and not d.w2 for d in marks)
        net.x.copy_(x)
        net.plan.run()
        _sync()
        outs.append(net.out.clone())
        launches.append(net.plan.time_tag(nets.TAG_PRIOR)[1])
        _sync()
    assert launches[1] - launches[0] == 4
    assert torch.equal(outs[0], outs[1])
    assert rel_l2(outs[0].cpu(), g["out"]) < 2e-5
