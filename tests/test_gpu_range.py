"""GPU tests of the range audit of the f16x2 window: csrc/range.hip against numpy (exact integer equality), the F16HI kind on
the plane tensors of a real plan, the completeness of ``audited()``, the audited pipeline (reads only, graph replay, nominal
inputs clean), the silent case - a tensor wholly below the window - seen and handled, the ``split=`` plumbing of the trainer
and the CLI, and the overflow case named.  Everything through the C-ABI."""
import argparse
import ctypes as C
import importlib
import logging

import numpy as np
import pytest
import torch

from conftest import pkg, seeded, tcm2_blocks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    lib = pkg("_lib")
    lib.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return lib


def _launch(L, rows, out, mode, keep):
    RA = pkg("rangeaudit")
    d = L.RangeDesc()
    d.out, d.out_rows, d.mode, d.blocks = out.data_ptr(), out.shape[0], mode, 1
    if rows:
        dev = torch.from_numpy(RA.table_of(rows)).to(DEV)
        keep.append(dev)
        d.rows, d.nrows, d.blocks = dev.data_ptr(), len(rows), RA.work_blocks(rows)
    L.launch(d)


def _counts(out):
    return out.cpu().numpy().view(np.uint32).astype(np.int64)


SIZES = [1, 3, 63, 64, 65, 257, 4099, 2 ** 20 + 5]


def test_f32_kernel_equals_numpy_exactly(L):
    """One launch over a table of fp32 tensors of n = 1 .. 2^20 + 5 elements (under one wave, tails that are no multiple of 4,
    many workgroups), values +-2^u m with u uniform over [-30, 20] and m in [1, 2), zeros, fp32 subnormals, +-inf and NaN planted,
    exponents 0 and 4; then a table whose every element lands in ONE bin (all lanes of every wave on one counter: the
    contention case).  Counts equal numpy's, integer for integer; clear + accumulate + accumulate gives twice the counts;
    rows that share an out_row add up."""
    RA = pkg("rangeaudit")
    rng = np.random.default_rng(11)
    tens, rows, want, keep = [], [], [], []
    for i, n in enumerate(SIZES):
        v = np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-30, 21, n)) * rng.choice([-1.0, 1.0], n)
        v = v.astype(np.float32)
        plant = [0.0, -0.0, 1e-40, -3e-45, np.inf, -np.inf, np.nan, 65504.0 / 16, 4096.0, 2.0 ** -18, np.float32(2.0 ** -6)]
        for j, p in enumerate(plant[:max(0, n - 1)]):
            v[(7 * j + 1) % n] = p
        e = (0, 4)[i & 1]
        t = torch.from_numpy(v).to(DEV)
        tens.append(t)
        rows.append(RA.make_row(t, L.RANGE_F32, e, None, i))
        want.append(RA.histogram(v, e))
    # the contention case: rows 8, 9 - every element in bin 16 (1 <= |x| < 2) resp. all zeros; row 10: an unaligned view
    hot = torch.from_numpy(rng.uniform(1.0, 2.0, 2 ** 18 + 3).astype(np.float32)).to(DEV)
    zeros = torch.zeros(70001, device=DEV)
    view = tens[-1][1:4098]
    for t, e in ((hot, 0), (zeros, 4), (view, 4)):
        rows.append(RA.make_row(t, L.RANGE_F32, e, None, len(rows)))
        want.append(RA.histogram(t.cpu().numpy(), e))
        tens.append(t)
    want = np.stack(want)
    assert want[8, 16] == hot.numel() and want[9, 0] == zeros.numel()
    out = torch.full((len(rows) + 2, 32), 77, dtype=torch.int32, device=DEV)
    _launch(L, None, out, L.RANGE_CLEAR, keep)
    assert not _counts(out).any()
    _launch(L, rows, out, L.RANGE_ACCUMULATE, keep)
    got = _counts(out)
    assert np.array_equal(got[:len(rows)], want) and not got[len(rows):].any()
    assert got[:len(rows)].sum(1).tolist() == [t.numel() for t in tens]
    _launch(L, rows, out, L.RANGE_ACCUMULATE, keep)
    assert np.array_equal(_counts(out)[:len(rows)], 2 * want)
    # two rows into one output row
    for r in rows[:2]:
        r.out_row = len(rows)
    _launch(L, rows[:2], out, L.RANGE_ACCUMULATE, keep)
    assert np.array_equal(_counts(out)[len(rows)], want[0] + want[1])


def test_argument_errors_before_any_launch(L):
    RA = pkg("rangeaudit")
    t = torch.zeros(16, device=DEV)
    out = torch.zeros(2, 32, dtype=torch.int32, device=DEV)
    good = RA.make_row(t, L.RANGE_F32, 4, None, 0)

    def bad(msg, **kw):
        r = L.RangeRow.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(r, k, v)
        with pytest.raises(L.PdseError, match=msg):
            _launch(L, [r], out, L.RANGE_ACCUMULATE, [])

    bad("null tensor", ptr=None)
    bad("unknown element kind", kind=2)
    bad("n < 0", n=-1)
    bad("out_row", out_row=2)
    bad("exponent", exp=200)
    d = L.RangeDesc()
    d.out, d.out_rows, d.mode, d.blocks = out.data_ptr(), 2, L.RANGE_ACCUMULATE, 1
    with pytest.raises(L.PdseError, match="null row table"):
        L.launch(d)
    d.rows = t.data_ptr()
    with pytest.raises(L.PdseError, match="zero rows"):
        L.launch(d)
    d.mode = 3
    with pytest.raises(L.PdseError, match="mode"):
        L.launch(d)
    d.mode, d.out = 0, None
    with pytest.raises(L.PdseError, match="null"):
        L.launch(d)
    torch.cuda.synchronize()
    assert not _counts(out).any()


@pytest.mark.parametrize("T", [40, 33])
def test_f16hi_kind_on_the_plane_tensors_of_a_real_plan(L, weights, T):
    """A small eps-net plan (B = 2, planes 2) run once: the device histogram of every hp_* and tcm_hs* tensor equals the host
    histogram of the same buffer un-packed by packing.hp_join / tcm2_join_h (hi plane, scaled units), and the element counts are
    the logical sizes - margins, pad frames, lo planes and the dump item are not counted.  T = 33: ragged tiles."""
    nets, P, RA = pkg("nets"), pkg("packing"), pkg("rangeaudit")
    B = 2
    net = nets.EpsNetPlan(nets.Ctx(DEV), weights("DiffUNet1"), B, T, time_cond=True, nsteps=1, planes=2)
    net.build_time()
    net.build_step(0)
    net.finish()
    net.x.copy_(seeded((B, 2, T, 161), 5))
    net.x_init.copy_(seeded((B, 2, T, 161), 6) * 0.3)
    net.tsteps.fill_(10.45)
    net.plan.run()
    torch.cuda.synchronize()
    aud = [a for a in net.audited() if a[2] == L.RANGE_F16HI]
    names = [a[0] for a in aud]
    assert sorted(names) == sorted(["hp_en%d" % k for k in range(2, 6)] + ["hp_de%d" % k for k in range(1, 6)] + ["hp_de5b"]
                                   + ["tcm_hs%d.%s" % (i, b) for i in range(2) for b in ("main", "mask")])
    rows = [RA.make_row(t, kind, e, box, i) for i, (_, t, kind, e, box) in enumerate(aud)]
    out = torch.zeros(len(rows), 32, dtype=torch.int32, device=DEV)
    _launch(L, rows, out, L.RANGE_ACCUMULATE, [])
    got = _counts(out)

    for i, (name, t, _, _, box) in enumerate(aud):
        raw = t.cpu().numpy().view(np.uint16)
        if name.startswith("hp_"):
            par = box["par_half"] != 0
            assert par == name.startswith("hp_en")
            v = P.hp_join(raw[:B], par=par)                                       # the logical tensor: its size is what must be counted
            F = raw.shape[4] - 2 * P.HP_F0
            assert v.shape == (B, 32, T, F)
            nat = raw[:B].take(P.hp_par_pos(raw.shape[4]), axis=4) if par else raw[:B]
            hi = nat[:, P.HP_T0:, :, 0, P.HP_F0:P.HP_F0 + F, :]                   # plane 0 over the index set hp_join keeps
        else:
            br = 1 if name.endswith(".mask") else 0
            v = P.tcm2_join_h(raw, B, T)[br]
            assert v.shape == (B, 64, T)
            hi = raw.reshape(P.tcm2_hs_shape(B, T, 2))[:, br, :, :, 0, P.TCM2_HS_PAD:P.TCM2_HS_PAD + T, :]
        assert hi.size == v.size and got[i].sum() == v.size, name
        # the stored hi plane, binned on the host: exact reference (hi is what decides the binade; lo is not read)
        assert got[i].tolist() == RA.histogram(P.f16_to_f32(hi)).tolist(), name
        # and hi is the fp16 nearest to the joined value wherever that is not a tie: the planes belong to the tensor hp_join returns
        assert np.abs(P.f16_to_f32(hi).astype(np.float64).sum() - np.ldexp(v.astype(np.float64), P.F16_ACT_EXP).sum()) <= 2.0 ** -10 * np.abs(np.ldexp(v.astype(np.float64), P.F16_ACT_EXP)).sum()
        assert got[i][1:].sum() > 0.9 * v.size                                   # a real tensor, not a buffer of zeros


def _f16x2_operand_ptrs(L, descs):
    """The activation pointers of the f16x2 launches of a recorded plan, read from the descriptors by the rules of the ABI
    (include/pdse.h): np == 2 bglu / tcm2 descs, korder == 5 gconv descs, np == 2 dense descs."""
    ptrs, n = [], 0
    blocks = tcm2_blocks(descs)
    for d in [d for d, _ in descs] + blocks:
        if isinstance(d, L.BgluDesc) and d.np == 2:
            ptrs += [d.hp] if d.hp else [d.x0.ptr, d.x1.ptr]
        elif isinstance(d, L.Tcm2Desc) and d.np == 2:
            ptrs += [d.x] + ([d.hs] if d.mode == 0 else [])
        elif isinstance(d, L.GconvDesc) and d.korder == 5:
            ptrs += [s.ptr for s in (d.in0, d.in1) if s.ptr]
        elif isinstance(d, L.DenseDesc) and d.np == 2:
            ptrs += [d.D]
        else:
            continue
        n += 1
    return ptrs, n


@pytest.mark.parametrize("name", ["GCRN", "DiffUNet", "aia_complex_trans_ri", "dual_aia_trans_merge_crm", "DiffUNet1"])
def test_audited_lists_every_f16x2_operand(L, weights, name):
    """B = 1, T = 24: every f16x2 launch recorded by the builder has its activation operand inside a tensor that audited()
    lists (no recording is run: the check is on descriptors)."""
    nets = pkg("nets")
    B, T = 1, 24
    ctx = nets.Ctx(DEV)
    if name == "GCRN":
        net = nets.GcrnPlan(ctx, weights(name), B, T, planes=2)
        net.build()
    elif name == "DiffUNet":
        net = nets.EpsNetPlan(ctx, weights(name), B, T, time_cond=False, planes=2)
        net.build_step(0)
    elif name == "DiffUNet1":
        net = nets.EpsNetPlan(ctx, weights(name), B, T, time_cond=True, nsteps=2, planes=2)
        net.build_time()
        net.build_step(0)
        net.build_step(1)
    else:
        net = {"aia_complex_trans_ri": nets.AiaPlan, "dual_aia_trans_merge_crm": nets.DualAiaPlan}[name](ctx, weights(name), B, T, planes=2)
        net.build()
    ptrs, nlaunch = _f16x2_operand_ptrs(L, net.descs)
    aud = net.audited()
    spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for _, t, *_ in aud]
    assert all(any(lo <= p < hi for lo, hi in spans) for p in ptrs)
    if name == "DiffUNet":           # the prior DiffUNet has no time conditioning: it runs the three-plane fallback, nothing to audit
        assert nlaunch == 0 and aud == []
    else:
        assert nlaunch > 0 and len(aud) > 0
        assert len({n for n, *_ in aud}) == len(aud) and not any("buf" in n for n, *_ in aud)       # every tensor has a name of its own


@pytest.fixture(scope="module")
def gcrn_pair(L, weights):
    """GCRN, B = 2, L = 6400, 6 steps: the same inputs through an audited and an un-audited pipeline (shared by the tests below)."""
    P = pkg("pipeline").SamplerPipeline
    B, L_ = 2, 6400
    wav, x_T = pkg("synth").synthetic_waveforms(B, L_, seed=21)
    wav, x_T = wav.to(DEV), x_T.to(DEV)
    plain = P(DEV, "GCRN", weights("GCRN"), weights("DiffUNet1"), B, L_=L_)
    aud = P(DEV, "GCRN", weights("GCRN"), weights("DiffUNet1"), B, L_=L_, audit=True)
    res_plain = plain.enhance(wav, x_T)
    plain.check()
    res_aud = aud.enhance(wav, x_T)
    aud.check(audit=True)
    rep = aud.range_report()
    return dict(plain=plain, aud=aud, res_plain=res_plain, res_aud=res_aud, rep=rep, wav=wav, x_T=x_T)


def test_audit_only_reads_and_adds_its_launches_only(L, gcrn_pair):
    g = gcrn_pair
    plain, aud = g["plain"], g["aud"]
    for a, b in zip(g["res_plain"], g["res_aud"]):
        assert torch.equal(a, b)
    # the un-audited plan holds the launches of its marked ranges and nothing else - what it held before the feature
    nrange = lambda p: [p.ranges[k][1] - p.ranges[k][0] for k in p.ranges]   # noqa: E731
    assert len(plain.descs) == sum(nrange(plain)) == len(plain.plan)
    assert not any(isinstance(d, L.RangeDesc) for d, _ in plain.descs)
    rd = [d for d, _ in aud.descs if isinstance(d, L.RangeDesc)]
    audited_ranges = ["prior"] + ["step%d" % n for n in range(aud.nsteps)]
    assert len(aud.descs) == len(plain.descs) + 1 + len(audited_ranges)
    assert [d.mode for d in rd] == [L.RANGE_CLEAR] + [L.RANGE_ACCUMULATE] * len(audited_ranges)
    assert isinstance(aud.descs[0][0], L.RangeDesc)
    for k in plain.ranges:
        extra = (1 if k == "stft" else 0) + (1 if k in audited_ranges else 0)
        assert aud.ranges[k][1] - aud.ranges[k][0] == plain.ranges[k][1] - plain.ranges[k][0] + extra
        assert isinstance(aud.descs[aud.ranges[k][1] - 1][0], L.RangeDesc) == (k in audited_ranges)
    everything = [d for d, _ in aud.descs if not isinstance(d, L.RangeDesc)]
    assert [type(d) for d in everything] == [type(d) for d, _ in plain.descs]
    # a second eager pass gives the same report (the table is cleared by the plan itself), and so does graph replay
    hist = lambda r: [row.hist for row in r]   # noqa: E731
    aud.enhance(g["wav"], g["x_T"])
    assert hist(aud.range_report()) == hist(g["rep"])
    out_g = aud.enhance(g["wav"], g["x_T"], graph=True)
    aud.check(audit=True)
    assert torch.equal(out_g[0], g["res_plain"][0]) and hist(aud.range_report()) == hist(g["rep"])
    # a pass that starts at a later range (sample()) starts from a cleared table as well
    feat = plain.feat.clone()
    s_plain = plain.sample(feat, g["x_T"])
    s_aud = aud.sample(feat, g["x_T"])
    assert torch.equal(s_plain[0], s_aud[0])
    assert [r.count for r in aud.range_report()] == [r.count for r in g["rep"]]


def test_nominal_inputs_are_clean(L, gcrn_pair):
    rep, aud = gcrn_pair["rep"], gcrn_pair["aud"]
    print(rep)
    assert rep.ok and rep.worst() is not None
    per_step = [n for n, *_ in aud.eps.audited()]
    per_step = [n for n in per_step if n != "x"] + ["x"]       # the diffusion state holds the step's output when the audit looks: last
    prior = [n for n, *_ in aud.prior.audited()]
    want = [("prior", n) for n in prior] + [("step%d" % s, n) for s in range(aud.nsteps - 1, -1, -1) for n in per_step]
    assert [(r.range, r.name) for r in rep] == want and aud.nsteps == 6 and len(per_step) >= 19
    for r in rep:
        assert r.count > 0 and r.max_binade is not None and -2 <= r.max_binade <= 14, r
        assert not r.below and not r.above


def _small_conv1_weights(weights, k=3):
    """DiffUNet1 weights whose encoder stage k computes its 1x1 input convolution 2^-12 times too small (weight and bias), with
    nothing compensating: the tensor the stage's gather reads, hp_en<k>, lies wholly below the fp16 window."""
    sd = dict(weights("DiffUNet1"))
    for f in ("weight", "bias"):
        sd["en.conv%d.conv1.%s" % (k, f)] = sd["en.conv%d.conv1.%s" % (k, f)] * 2.0 ** -12
    return sd


def _trainer(sd_prior, sd, tmp_path, **kw):
    ns = argparse.Namespace
    return pkg("trainer").ComplexDDPMTrainer(
        ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav=str(tmp_path)),
        ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
        device=DEV, prior_state_dict=sd_prior, ddpm_state_dict=sd, exclusive=False, **kw)


def test_a_tensor_wholly_below_the_window_is_seen_and_handled(L, weights, tmp_path, caplog):
    """The silent case.  Which quantity was checked: the obvious recipe - one encoder stage's GATHER weights times 2^-12 - does not
    empty the window: in float64 (oracle/restate.py, B = 1, T = 24, the inputs below) the following stage's conv1 tensor keeps
    max |x| between 0.59 and 0.99 for every stage 1 .. 4 and for 2^-20 as well (profiles/range_audit_parity.txt), because the gather, conv2, BatchNorm, time and
    conv1 biases do not shrink with the weights.  What does is the conv1 of a stage itself: encoder stage 3's 1x1 input convolution
    (weight and bias) times 2^-12, nothing compensating.  The test first confirms with the float64 oracle that this tensor - the one
    the kernels keep as hp_en3 - has max |x| < 2^-6 (it is about 2^-10), then asks the device."""
    R = importlib.import_module("oracle.restate")
    F = torch.nn.functional
    sd = _small_conv1_weights(weights, 3)
    B, T = 2, 24
    feat, x_T = seeded((B, 2, T, 161), 41), seeded((B, 2, T, 161), 42)
    with torch.no_grad():                                                     # float64: conv1 of encoder stage 3 on a step-like input
        s64 = {k: v.double() for k, v in sd.items()}
        x = F.conv2d(torch.cat((x_T, 0.3 * feat), 1).double(), s64["preprocess.conv.weight"], s64["preprocess.conv.bias"])
        temb = R.time_embedding(s64, torch.full((B,), 10.45).double(), R.build_time_table(50))
        for k in (1, 2, 3):
            x = F.pad(x, (0, 0, 1, 0)) + F.linear(temb, s64["en.tp%d.weight" % k], s64["en.tp%d.bias" % k])[:, :, None, None]
            if k == 3:
                c1 = F.conv2d(x, s64["en.conv3.conv1.weight"], s64["en.conv3.conv1.bias"])
            else:
                x = R._prelu(s64, "en.en%d.1" % k, R._bn(s64, "en.en%d.0" % k, R.biconvglu(s64, "en.conv%d" % k, x)))
    assert 0 < float(c1.abs().max()) < 2.0 ** -6

    P = pkg("pipeline").SamplerPipeline
    pipe = P(DEV, "GCRN", weights("GCRN"), sd, B, T=T, audit=True)
    spec16 = pipe.sample(feat.to(DEV), x_T.to(DEV))[0]
    pipe.check()                                                              # the hole: finite output, nothing raised
    assert torch.isfinite(spec16).all()
    rep = pipe.range_report()
    assert not rep.ok and rep.above() == []
    assert [(r.name, r.range) for r in rep.below()] == [("hp_en3", "step%d" % s) for s in range(pipe.nsteps - 1, -1, -1)]
    assert rep.worst().name == "hp_en3" and all(r.below_frac == 1.0 and r.max_binade < -2 for r in rep.below())
    with pytest.raises(L.PdseRangeError, match=r"hp_en3 in step5"):
        pipe.check(audit=True)

    ref = P(DEV, "GCRN", weights("GCRN"), sd, B, T=T, split="bf16x3")
    want = ref.sample(feat.to(DEV), x_T.to(DEV))[0]
    ref.check()
    with caplog.at_level(logging.WARNING):
        tr = _trainer(weights("GCRN"), sd, tmp_path, audit=True)
        got = tr.sample(feat, x_T=x_T)
    assert any("hp_en3" in r.getMessage() and "bf16x3" in r.getMessage() for r in caplog.records)
    assert len(tr._range_fallback) == 1 and torch.equal(got, want)
    assert next(iter(tr._pipes.values())).split == "bf16x3"
    got2 = tr.sample(feat, x_T=x_T)                                           # stays on the fallback, same bits
    assert torch.equal(got2, want) and len(tr._pipes) == 1
    # without the audit the trainer returns what it always returned: the f16x2 result, no exception, no fallback
    tr0 = _trainer(weights("GCRN"), sd, tmp_path)
    assert not tr0.audit
    got0 = tr0.sample(feat, x_T=x_T)
    assert torch.equal(got0, spec16) and not tr0._range_fallback
    assert not any(isinstance(d, L.RangeDesc) for d, _ in next(iter(tr0._pipes.values())).descs)
    # a clean geometry is audited until it came back clean once, then keeps its plan
    tr1 = _trainer(weights("GCRN"), weights("DiffUNet1"), tmp_path, audit=True)
    a = tr1.sample(feat, x_T=x_T)
    assert len(tr1._audit_clean) == 1 and not tr1._range_fallback
    assert torch.equal(tr1.sample(feat, x_T=x_T), a) and next(iter(tr1._pipes.values())).audited


def test_split_plumbing_of_the_trainer_and_the_cli(L, weights, tmp_path, monkeypatch):
    P = pkg("pipeline").SamplerPipeline
    B, T = 1, 24
    feat, x_T = seeded((B, 2, T, 161), 51), seeded((B, 2, T, 161), 52)
    ref = P(DEV, "GCRN", weights("GCRN"), weights("DiffUNet1"), B, T=T, split="bf16x3")
    want = ref.sample(feat.to(DEV), x_T.to(DEV))[0]
    tr = _trainer(weights("GCRN"), weights("DiffUNet1"), tmp_path, split="bf16x3")
    got = tr.sample(feat, x_T=x_T)
    pipe = next(iter(tr._pipes.values()))
    assert pipe.split == "bf16x3" and pipe.eps.planes == 3 and torch.equal(got, want) and not tr._range_fallback
    assert _trainer(weights("GCRN"), weights("DiffUNet1"), tmp_path).split is None
    with pytest.raises(ValueError):
        _trainer(weights("GCRN"), weights("DiffUNet1"), tmp_path, split="fp8")
    # the CLI: --split / --audit-range reach the trainer through args
    main = pkg("main")
    (tmp_path / "conf").mkdir()
    (tmp_path / "conf" / "diff.yml").write_text("model:\n  name: GCRN\ntrain:\n  fft_num: 320\n  win_size: 320\n  win_shift: 160\n  feat_type: sqrt\n")
    monkeypatch.chdir(tmp_path)
    args, config = main.parse_args_and_config(["--split", "bf16x3", "--audit-range", "--assets", str(tmp_path / "a")])
    assert args.split == "bf16x3" and args.audit_range is True
    tr2 = pkg("trainer").ComplexDDPMTrainer(args, config, device=DEV, prior_state_dict=weights("GCRN"), ddpm_state_dict=weights("DiffUNet1"),
                                            exclusive=False)
    assert tr2.split == "bf16x3" and tr2.audit
    got2 = tr2.sample(feat, x_T=x_T)
    p2 = next(iter(tr2._pipes.values()))
    assert p2.split == "bf16x3" and p2.audit and not p2.audited and torch.equal(got2, want)
    args0, _ = main.parse_args_and_config(["--assets", str(tmp_path / "a")])
    assert args0.split is None and args0.audit_range is False
    # new weights deserve a new verdict: load_checkpoint clears the fallback set and the clean set
    tr2._range_fallback.add(("some", "geometry"))
    tr2._audit_clean.add(("some", "geometry"))
    ck = tmp_path / "ck"
    ck.mkdir()
    torch.save([weights("GCRN"), None, weights("DiffUNet1")], str(ck / "best_checkpoint.pth"))
    tr2.args.checkpoint = str(ck)
    tr2._load_checkpoint()
    assert not tr2._range_fallback and not tr2._audit_clean and not tr2._pipes and not tr2._hits


def test_overflow_is_named_by_the_audit(L, weights):
    """The overflow recipe of test_gpu_f16x2.py (conv1 bias of encoder stage 3 + 3e4: far beyond +-4094) on an audited pipeline:
    the report has ``above`` rows, the first of them is hp_en3 in the first step, and check() names it."""
    sd = dict(weights("DiffUNet1"))
    sd["en.conv3.conv1.bias"] = sd["en.conv3.conv1.bias"] + 3.0e4
    wav, x_T = pkg("synth").synthetic_waveforms(2, 4000, seed=77)
    pipe = pkg("pipeline").SamplerPipeline(DEV, "GCRN", weights("GCRN"), sd, 2, L_=4000, audit=True)
    pipe.enhance(wav.to(DEV), x_T.to(DEV))
    rep = pipe.range_report()
    top = rep.above()
    assert top and (top[0].name, top[0].range) == ("hp_en3", "step5") and top[0].hist[31] > 0
    assert not any(r.above for r in rep if r.range == "prior")
    with pytest.raises(L.PdseRangeError, match=r"fp16.*|hp_en3") as ei:
        pipe.check()
    assert "hp_en3 of step5" in str(ei.value) and "fp16" in str(ei.value)


def test_plan_file_round_trip_carries_the_audit(L, weights, tmp_path):
    """An audited pipeline saved to a plan file, loaded by pdse_plan_load (which rebases the row tables of the range ops) and run
    by pdse_enhance: the region range_hist of the loaded plan equals the range_report() of the recording pipeline on the same
    inputs, row for row, and so do the outputs."""
    pf = pkg("planfile")
    B, L_ = 1, 2560
    wav, x_T = pkg("synth").synthetic_waveforms(B, L_, seed=9)
    wav, x_T = wav.to(DEV), x_T.to(DEV)
    pipe = pkg("pipeline").SamplerPipeline(DEV, "GCRN", weights("GCRN"), weights("DiffUNet1"), B, L_=L_, audit=True)
    path = pf.save_pipeline(str(tmp_path / "audited.plan"), pipe)                # before the first run: buffers as the builders left them
    want_wav, want_spec = pipe.enhance(wav, x_T)
    pipe.check(audit=True)
    rep = pipe.range_report()
    assert len(rep) == len(pipe.range_rows) > 0

    lib = L.load()
    plan = C.c_void_p()
    L.check(lib.pdse_plan_load(path.encode(), C.byref(plan)), "pdse_plan_load")
    try:
        out, spec = torch.empty_like(wav), torch.empty_like(x_T)
        vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(2):                                                       # the second call: the plan clears its own table
            L.check(lib.pdse_enhance(plan, vp(wav), vp(x_T), vp(out), vp(spec), st), "pdse_enhance")
        torch.cuda.synchronize()
        ptr, nbytes = C.c_void_p(), C.c_uint64()
        L.check(lib.pdse_plan_region(plan, b"range_hist", C.byref(ptr), C.byref(nbytes)), "pdse_plan_region")
        assert nbytes.value == pipe.range_hist.numel() * 4 and ptr.value != pipe.range_hist.data_ptr()

        class Region:
            __cuda_array_interface__ = {"shape": (nbytes.value // 4,), "typestr": "<i4", "data": (ptr.value, False), "version": 2}

        hist = torch.as_tensor(Region(), device=DEV).cpu().numpy().view(np.uint32).reshape(-1, 32)
        assert [h.tolist() for h in hist[:len(rep)]] == [r.hist for r in rep] and not hist[len(rep):].any()
        assert torch.equal(out, want_wav) and torch.equal(spec, want_spec)
    finally:
        lib.pdse_plan_destroy(plan)
