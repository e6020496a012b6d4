"""CPU: what nets.GcrnPlan records for the fused decoder phases (GcrnPlan.fuse_phases).  The mark is two integers on the even-bin
descriptor (include/pdse.h: p1mask / Fout1 with w2 == NULL); nothing else of any descriptor changes, so the interpreter
(tests/emu.py), which runs every descriptor as a launch of its own, gives the same result for either setting."""
import numpy as np
import torch

import emu
from conftest import pkg, seeded


def _plan(weights, fuse, monkeypatch, **kw):
    nets = pkg("nets")
    monkeypatch.setattr(nets.GcrnPlan, "fuse_phases", fuse)
    ctx = nets.Ctx("cpu")
    net = nets.GcrnPlan(ctx, weights("GCRN"), 2, 6, **kw)
    net.build()
    return ctx, net


def _gconvs(net):
    L = pkg("_lib")
    return [d for d, _ in net.descs if isinstance(d, L.GconvDesc)]


def test_marks_name_the_odd_phase_of_the_small_stages(weights, monkeypatch):
    _, net = _plan(weights, True, monkeypatch)
    ds = _gconvs(net)
    marked = [i for i, d in enumerate(ds) if d.p1mask]
    assert len(marked) == 4                                      # conv3_t and conv2_t of both decoders
    for i in marked:
        d, e = ds[i], ds[i + 1]
        assert d.korder == e.korder == 5 and d.Cout == e.Cout and d.Cout <= 32 and not d.w2 and not e.w2 and e.p1mask == 0
        assert d.ntaps == 2 and e.ntaps == 1 and (d.tap_dt[0], d.tap_df[0]) == (e.tap_dt[0], e.tap_df[0]) == (0, 0)
        assert d.Fout1 == e.Fout and d.Fout - e.Fout in (0, 1) and (d.B, d.Tout) == (e.B, e.Tout)
        for a, b in ((d.in0, e.in0), (d.in1, e.in1)):
            assert (a.ptr, a.sb, a.sc, a.st, a.sf, a.C, a.act, a.blk) == (b.ptr, b.sb, b.sc, b.st, b.sf, b.C, b.act, b.blk)
        assert e.out == d.out and e.out_off - d.out_off == d.out_sf // 2
    # 64 and 128 output channels: two launches, no mark
    assert all(not d.p1mask for d in ds if d.korder == 5 and d.Cout > 32)


def test_switch_off_and_other_forms_record_no_mark(weights, monkeypatch):
    _, off = _plan(weights, False, monkeypatch)
    assert not any(d.p1mask or d.Fout1 for d in _gconvs(off))
    for kw in (dict(planes=3), dict(planes=1), dict(split_bf16=False)):          # bf16x3, the bf16 mode, fp32: what they had
        _, net = _plan(weights, True, monkeypatch, **kw)
        assert not any(d.p1mask or d.Fout1 for d in _gconvs(net)), kw


def test_descriptors_differ_in_the_mark_only_and_replay_alike(weights, monkeypatch):
    x = seeded((2, 2, 6, 161), 11)
    outs = []
    for fuse in (True, False):
        ctx, net = _plan(weights, fuse, monkeypatch)
        net.x.copy_(x)
        emu.run(net.descs, ctx.all_tensors())
        outs.append(net.out.clone())
    assert torch.equal(outs[0], outs[1]) and bool(np.isfinite(outs[0].numpy()).all())
