"""CPU: the window schedule of long recordings (longplan.py) and the receptive fields the plan builders report, the eps-net's
held against the float64 oracle by perturbing one input frame."""
import numpy as np
import pytest
import torch

from conftest import pkg


def _check_schedule(T, W, Hl, Hr):
    wins = pkg("longplan").windows(T, W, Hl, Hr)
    if T <= W:
        assert wins == [(0, 0, T)]
        return wins
    assert wins[0][0] == 0 and wins[-1][0] + W == T                     # the file's edges are window edges: no invented halo
    at = 0
    for a, lo, hi in wins:
        assert 0 <= a <= T - W, (T, a)
        assert lo == at and lo < hi, (T, wins)                          # the kept ranges partition [0, T) in order
        assert lo >= a + Hl or (a == 0 and lo == 0), (T, a, lo)
        assert hi <= a + W - Hr or (a + W == T and hi == T), (T, a, hi)
        at = hi
    assert at == T
    return wins


def test_windows_properties_sweep():
    Hl, Hr, W = 5, 3, 32
    for T in list(range(1, 4 * W)) + [W, W + 1, 2 * W - Hl - Hr - 1, 2 * W - Hl - Hr, 2 * W - Hl - Hr + 1, 10 * W + 7]:
        _check_schedule(T, W, Hl, Hr)
    assert len(_check_schedule(W + 1, W, Hl, Hr)) == 2
    assert len(_check_schedule(2 * W - Hl - Hr - 1, W, Hl, Hr)) == 2      # the clamped last window still owns >= H_left of halo
    assert len(_check_schedule(2 * W + 37, W, Hl, Hr)) >= 3
    for W2, H in ((832, (388, 378)), (2048, (388, 378)), (64, (0, 0)), (96, (40, 0)), (96, (0, 40))):
        for T in (W2, W2 + 1, 2 * W2 - sum(H) - 1, 2 * W2 + 37, 7 * W2 + 5):
            _check_schedule(T, W2, *H)


def test_windows_refuses_a_window_inside_the_field():
    lp = pkg("longplan")
    for W, Hl, Hr in ((8, 5, 3), (7, 5, 3), (766, 388, 378)):
        with pytest.raises(ValueError, match="receptive field"):
            lp.windows(1000, W, Hl, Hr)
    assert lp.windows(1000, 767, 388, 378)
    for bad in (0, 31, 33, -32, 2.5, True, "64"):
        with pytest.raises(ValueError, match="multiple of 32"):
            lp.window_arg(bad)
    assert lp.window_arg(None) is None and lp.window_arg(64) == 64
    assert lp.DEFAULT_WINDOW % lp.FRAME_TILE == 0 and lp.DEFAULT_WINDOW > 2 * (388 + 378)
    assert lp.round_up(830) == 832 and lp.round_up(832) == 832


def test_carried_windows_are_consecutive():
    lp = pkg("longplan")
    assert lp.carried(7, 3) == [(0, 0, 3), (3, 3, 6), (6, 6, 7)]
    assert lp.carried(6, 3) == [(0, 0, 3), (3, 3, 6)]
    assert lp.carried(2, 3) == [(0, 0, 2)]


def test_window_conflicts_name_the_option():
    lp = pkg("longplan")
    lp.window_conflicts(ragged=False, members=1, inflight=1, per_channel=False, objective=False, plan_file=False)
    for kw, word in ((dict(ragged=True), "ragged"), (dict(members=2), "members=2"), (dict(inflight=2), "inflight=2"),
                     (dict(per_channel=True), "per_channel"), (dict(objective=True), "objective"), (dict(plan_file=True), "plan_file")):
        with pytest.raises(ValueError, match=word):
            lp.window_conflicts(**kw)


def test_pipeline_and_cli_refuse_combinations(weights):
    pipeline = pkg("pipeline")
    gs, ds = weights("GCRN"), weights("DiffUNet1")
    mk = lambda prior="GCRN", sd=gs, **kw: pipeline.SamplerPipeline("cpu", prior, sd, ds, 1, L_=2560, window=64, **kw)   # noqa: E731
    for kw in (dict(ragged=True), dict(members=2), dict(verdict=True), dict(objective=True), dict(label=True), dict(audit=True)):
        with pytest.raises(ValueError, match="window"):
            mk(**kw)
    for prior in ("aia_complex_trans_ri", "dual_aia_trans_merge_crm"):
        with pytest.raises(ValueError, match="attends"):
            mk(prior=prior, sd={})
    with pytest.raises(ValueError, match="multiple of 32"):
        pipeline.SamplerPipeline("cpu", "GCRN", gs, ds, 1, L_=2560, window=50)
    with pytest.raises(ValueError, match="L_"):
        pipeline.SamplerPipeline("cpu", "GCRN", gs, ds, 1, T=17, window=64)
    main = pkg("main")
    for argv in (["--generate", "--window", "64", "--batch", "2"], ["--generate", "--window", "64", "--inflight", "2"],
                 ["--generate", "--window", "64", "--per-channel"], ["--generate", "--window", "64", "--members", "2"],
                 ["--eval", "--window", "64"], ["--generate", "--window", "50"]):
        with pytest.raises(SystemExit):
            main.parse_args_and_config(argv)


def test_window_none_records_todays_plan(weights):
    """window=None, and a window the recording fits in, record the operator sequence of a pipeline without the option."""
    pipeline = pkg("pipeline")
    gs, ds = weights("GCRN"), weights("DiffUNet1")
    kinds = lambda p: [(type(d).__name__, tag) for d, tag in p.descs]      # noqa: E731
    base = pipeline.SamplerPipeline("cpu", "GCRN", gs, ds, 1, L_=2560)
    for w in (None, 32):
        p = pipeline.SamplerPipeline("cpu", "GCRN", gs, ds, 1, L_=2560, window=w)
        assert p.long is None and kinds(p) == kinds(base) and p.ranges == base.ranges
    L = pkg("_lib")
    gl = [d for d, _ in base.descs if isinstance(d, L.GlstmDesc)]
    assert gl and all(d.state_in is None and d.state_out is None for d in gl)


def test_receptive_fields_from_the_builders(weights):
    nets = pkg("nets")
    ctx = nets.Ctx("cpu")
    eps = nets.EpsNetPlan(ctx, weights("DiffUNet1"), 1, 8, nsteps=1)
    st = eps.time_stages()
    assert len(st) == 5 + 18 + 5 and [s[0] for s in st[:5]] == ["en%d" % k for k in range(1, 6)]
    assert eps.receptive_field() == (388, 378)                             # 5 + 3 * 2 * 63 + 5 back, 3 * 2 * 63 ahead
    prior = nets.EpsNetPlan(nets.Ctx("cpu"), weights("DiffUNet"), 1, 8, time_cond=False)
    assert prior.receptive_field() == (388, 378) and not prior.carries_state
    g = nets.GcrnPlan(nets.Ctx("cpu"), weights("GCRN"), 1, 8)
    assert g.receptive_field() == (0, 0) and g.carries_state is True
    assert nets.AiaPlan.receptive_field(object()) is None and nets.DualAiaPlan.receptive_field(object()) is None
    # not a constant: another layer table gives another field
    class Short(nets.EpsNetPlan):
        TCM_STACKS, TCM_DILATIONS = 1, (1, 2)

    short = Short.__new__(Short)
    short.sd = eps.sd
    assert len(short.time_stages()) == 5 + 2 + 5 and short.receptive_field() == (5 + 6 + 5, 6)


def test_eps_receptive_field_against_the_float64_oracle(weights):
    """Perturb one frame of x in oracle/restate.py's float64 eps-net: the output frames that change are exactly
    [t0 - H_right, t0 + H_left] clipped to the file - the field is neither under- nor over-stated.  T = H_left + H_right + 9."""
    from oracle import restate as R

    nets = pkg("nets")
    sd32 = weights("DiffUNet1")
    Hl, Hr = nets.EpsNetPlan(nets.Ctx("cpu"), sd32, 1, 8, nsteps=1).receptive_field()
    T = Hl + Hr + 9
    sd = {k: v.double() for k, v in sd32.items()}
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 2, T, 161, generator=g, dtype=torch.float64)
    x_init = torch.randn(1, 2, T, 161, generator=g, dtype=torch.float64)
    t = torch.tensor([3])
    t0 = Hr + 4                                    # both ends of the field lie inside the file: [4, t0 + H_left = T - 5]
    xp = x.clone()
    xp[:, :, t0] += 1.0
    with torch.no_grad():
        base = R.diffunet1_forward(sd, x, x_init, t)
        pert = R.diffunet1_forward(sd, xp, x_init, t)
    changed = ((base - pert).abs().amax(dim=(0, 1, 3)) > 0).numpy()
    want = np.zeros(T, dtype=bool)
    want[max(0, t0 - Hr):min(T, t0 + Hl + 1)] = True
    assert changed.any() and not changed.all(), "whole-length dependence"
    first, last = int(np.flatnonzero(changed)[0]), int(np.flatnonzero(changed)[-1])
    print("changed frames [%d, %d], stated [%d, %d]" % (first, last, t0 - Hr, t0 + Hl))
    assert (first, last) == (t0 - Hr, t0 + Hl)
    assert not changed[~want].any()
