"""CPU: (1) the statement of the grouped LSTM in tests/helpers/lstm_refs.py against a module assembled here from
torch.nn.LSTM and torch.nn.LayerNorm in double; (2) every case of tests/helpers/lstm_cases.py - the descriptors
tests/test_gpu_lstm_ops.py launches - replayed on tests/emu.py (run_lstm, run_glstm, run_glstmp, run_ln) and held to the
float64 reference by the very check the GPU file applies, which pins the packing, the descriptor builder and the checks
without a GPU; (3) the regimes' stated properties on the float64 reference; (4) that nets.GcrnPlan hands the packing
functions the state-dict keys the case helper hands them (the packers themselves are held by (2) and by the GPU file; byte
identity of the plans with earlier ones by the plan tests of tests/test_host_logic.py)."""
import numpy as np
import pytest
import torch
from torch import nn

import emu
from conftest import pkg
from helpers import lstm_cases as G
from helpers import lstm_refs as R

TOL = dict(atol=1e-12, rtol=1e-12)
F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------ the reference against torch
class TorchGLSTM(nn.Module):
    """Two layers of two independent LSTMs over the halves of the features; the first layer's outputs stacked on a new last
    dim and flattened, the second layer's concatenated; LayerNorm(1024) behind each layer."""

    def __init__(self):
        super().__init__()
        self.lstm_list1 = nn.ModuleList([nn.LSTM(R.H, R.H, 1, batch_first=True) for _ in range(R.G)])
        self.lstm_list2 = nn.ModuleList([nn.LSTM(R.H, R.H, 1, batch_first=True) for _ in range(R.G)])
        self.ln1, self.ln2 = nn.LayerNorm(R.G * R.H), nn.LayerNorm(R.G * R.H)

    def forward(self, x):
        y1 = torch.stack([m(c)[0] for m, c in zip(self.lstm_list1, torch.chunk(x, R.G, dim=-1))], dim=-1).flatten(-2)
        y2 = torch.cat([m(c)[0] for m, c in zip(self.lstm_list2, torch.chunk(self.ln1(y1), R.G, dim=-1))], dim=-1)
        return y1, y2, self.ln2(y2)


@pytest.mark.parametrize("B,T,seed", [(1, 1, 1), (3, 5, 2), (2, 12, 3)])
def test_ref_matches_torch_lstm_and_layernorm(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    m = TorchGLSTM().double()
    with torch.no_grad():
        for name, t in m.named_parameters():
            t.copy_(torch.randn(t.shape, generator=g, dtype=F64) * (1.0 if t.dim() == 1 else 2.0 / np.sqrt(R.H)))
    p = {k: v.detach() for k, v in m.state_dict().items()}
    x = torch.randn(B, T, R.G * R.H, generator=g, dtype=F64)
    with torch.no_grad():
        y1, y2, out = m(x)
    gx1 = torch.stack([R.project(c, p, "lstm_list1", i) for i, c in enumerate(torch.chunk(x, R.G, dim=-1))], 0)
    got = R.block(gx1, p, ln2=True)
    torch.testing.assert_close(got["y1"], y1, **TOL)
    torch.testing.assert_close(got["y"], y2, **TOL)
    torch.testing.assert_close(got["out"], out, **TOL)
    # one layer from its projections, both ways of joining the groups
    h = R.layer(gx1, [p["lstm_list1.%d.weight_hh_l0" % i] for i in range(R.G)])
    torch.testing.assert_close(R.interleave(h), y1, **TOL)
    torch.testing.assert_close(R.concat(h)[..., R.H:], y1[..., 1::2], **TOL)


@pytest.mark.parametrize("case", G.LN, ids=G.by_id(G.LN))
def test_ref_strided_store_is_a_permuted_layernorm(case):
    """ln_store against nn.LayerNorm followed by torch's own reshapes: r = 1 -> [B, C, T], r > 1 -> [B, C, T, r]; blk 8:
    the channels in blocks of 8, innermost."""
    x, gam, bet = G.ln_params(case)
    s, n = G.ln_strides(case)
    B, T, N, r = case["B"], case["T"], case["N"], case["r"]
    ln = nn.LayerNorm(N, eps=G.EPS).double()
    with torch.no_grad():
        ln.weight.copy_(gam)
        ln.bias.copy_(bet)
        y = ln(x.double())
    C = -(-N // r)
    Cp = -(-C // 8) * 8 if s["blk"] else C
    full = torch.full((B, T, Cp * r), float("nan"), dtype=F64)
    full[..., :N] = y
    want = full.view(B, T, Cp, r).permute(0, 2, 1, 3)                       # [B, C, T, r]
    if s["blk"]:
        want = want.reshape(B, Cp // 8, 8, T, r).permute(0, 1, 3, 4, 2)     # [B, C/8, T, r, 8]
    got = R.ln_store(x, gam, bet, n, s, G.EPS)
    assert got.numel() == want.numel()
    torch.testing.assert_close(got, want.reshape(-1), equal_nan=True, **TOL)


# ------------------------------------------------------------------ the case table on the emulator
def _replay(case, **kw):
    b = G.build(case, "cpu", **kw)
    with np.errstate(over="ignore", invalid="ignore"):
        emu.RUNNERS[type(b.desc)](b.desc, emu.Mem(G.tensors(b)))
    return b


@pytest.mark.parametrize("case", G.LSTM + G.GLSTM + G.GLSTMP, ids=G.by_id(G.LSTM + G.GLSTM + G.GLSTMP))
def test_emulator_lstm(case):
    b = _replay(case)
    G.check(case["id"], G.read(b), G.ref(case, F64), G.ref(case, F32), case["regime"])


@pytest.mark.parametrize("case", G.LN, ids=G.by_id(G.LN))
def test_emulator_layernorm(case):
    b = _replay(case)
    at = b.pos.reshape(-1)
    assert at.unique().numel() == at.numel(), "two elements stored at one place"
    G.check(case["id"], G.read(b).reshape(-1), G.ref(case, F64)[at], G.ref(case, F32)[at])


def test_builder_variants_on_the_emulator():
    """What the structural GPU tests rely on: NaN in the padded rows changes nothing, item B - 1 alone has the same inputs
    (same weights, its own projections), a shorter T runs on another case's scratch."""
    for name in ("lstm_B31_T7_tiny_cat", "glstm_s1_B31_T3_sat_il", "glstmp_B3_T3_sat_cat"):
        case = G.find(name)
        b = _replay(case)
        whole = G.read(b)
        assert G.same_bits(G.read(_replay(case, pad_nan=True)), whole)
        alone = G.variant(case, B=1, first_item=case["B"] - 1)
        assert torch.equal(G.projections(alone)[:, 0], G.projections(case)[:, case["B"] - 1])
        torch.testing.assert_close(G.ref(alone, F64)[:, 0], G.ref(case, F64)[:, case["B"] - 1], **TOL)
        short = G.variant(case, T=case["T"] - 2)
        assert G.same_bits(G.read(_replay(short, scr=b.scr)), G.read(_replay(short)))


# ------------------------------------------------------------------ the regimes are what they say
def test_case_table_reaches_what_it_names():
    """Every B / T edge and every regime at every kernel, both layouts, both slice counts."""
    def has(cases, key):
        return {c[key] for c in cases}
    assert {(c["B"], c["Bp"]) for c in G.LSTM} == {(1, 32), (31, 32), (33, 64)} and has(G.LSTM, "T") == {1, 2, 7}
    assert has(G.LSTM, "regime") == {"n01", "hot", "sat", "tiny"}
    assert {(c["B"], c["Bp"]) for c in G.GLSTM} >= {(1, 32), (31, 32), (32, 32), (33, 64)} and has(G.GLSTM, "T") == {1, 2, 3, 7, 33, 160}
    assert {(c["B"], c["Bp"]) for c in G.GLSTMP} == {(1, 32), (2, 32), (3, 32), (4, 32), (5, 32), (8, 32), (3, 3)}
    assert has(G.GLSTMP, "T") == {1, 2, 3, 7, 33, 160}
    for cases in (G.GLSTM, G.GLSTMP):
        assert has(cases, "regime") == set(G.REGIMES)
    for s in (1, 2):
        assert {c["regime"] for c in G.GLSTM if c["slices"] == s} == set(G.REGIMES)
    for cases in (G.LSTM, G.GLSTM, G.GLSTMP):
        assert has(cases, "layout") == {"il", "cat"}
    assert {c["B"] * c["T"] for c in G.LN} == {1, 3, 5} and has(G.LN, "N") == {1, 63, 65, 1000, 1024}
    assert has(G.LN, "r") == {1, 4} and has(G.LN, "blk") == {0, 8} and has(G.LN, "dist") == {"n01", "m64"}
    assert len(G.ALL) <= 60
    for p in (G.natural(c) for c in (G.LSTM[0], G.GLSTM[0], G.GLSTMP[0])):
        gam = p["ln1.weight"]
        assert (gam[:R.H] == 0).sum() == 2 and (gam[R.H:] == 0).sum() == 2 and (gam < 0).any() and (gam > 0).any()


@pytest.mark.parametrize("case", [c for c in G.GLSTM + G.GLSTMP if c["regime"] in ("offset", "flat")],
                         ids=G.by_id([c for c in G.GLSTM + G.GLSTMP if c["regime"] in ("offset", "flat")]))
def test_offset_and_flat_are_what_they_say(case):
    """Layer 1's outputs in the float64 reference: |mean| >= 0.6 over the 1024 features and variance <= 1e-2 (offset),
    <= 1e-5 (flat: below eps), at every frame t >= 4 - and in fact at every frame but the first."""
    y1 = G.ref_y1(case)
    mean, var = y1.mean(-1), y1.var(-1, unbiased=False)
    lim = 1e-2 if case["regime"] == "offset" else 1e-5
    assert bool((mean[:, 4:].abs() >= 0.6).all()) and bool((var[:, 4:] <= lim).all())
    assert bool((mean[:, 1:].abs() >= 0.6).all()) and bool((var[:, 1:] <= lim).all())
    if case["regime"] == "offset":
        assert bool((var > 1e-4).all()), "offset is meant to sit above eps"


@pytest.mark.parametrize("case", [c for c in G.LSTM + G.GLSTM + G.GLSTMP if c["regime"] in ("sat", "tiny", "hot")],
                         ids=G.by_id([c for c in G.LSTM + G.GLSTM + G.GLSTMP if c["regime"] in ("sat", "tiny", "hot")]))
def test_sat_tiny_and_hot_are_what_they_say(case):
    y = G.ref(case, F64)                                            # [G, B, T, H]
    if case["regime"] == "tiny":                                    # |h| = sigmoid(o) |tanh(c)| with |c| ~ 1e-4
        assert 1e-5 < float(y.abs().median()) < 3e-4 and float(y.abs().max()) < 1e-2
    elif case["regime"] == "sat":
        assert np.isinf(np.exp(np.float32(G._SAT))) and np.exp(np.float32(-G._SAT)) > 0
        # units with the output gate at -100 give h = 0 (3.7e-44 at the most), those with the input gate at -100 and no
        # history c = 0; a unit with g at +-100 and the other gates free is sigmoid(o) tanh(+-sigmoid(i) ..): finite, |h| < 1
        assert float(y[..., 7::8].abs().max()) < 1e-40
        assert float(y[:, :, 0, 4::8].abs().max()) < 1e-40
        assert float(y.abs().max()) < 1.0
    elif case["T"] > 1:                                             # the recurrent term is as large as the O(1) projections
        layer = "lstm_list1" if case["kernel"] == "lstm" else "lstm_list2"
        p = G.natural(case)
        rec = torch.stack([y[g, :, :-1] @ torch.as_tensor(p["%s.%d.weight_hh_l0" % (layer, g)]).double().T for g in range(R.G)], 0)
        assert float(rec.std()) > 0.8


# ------------------------------------------------------------------ the packing against nets.GcrnPlan
@pytest.mark.parametrize("form", ["generic", "wavefront", "persistent"])
def test_packed_operands_match_gcrn_plan(weights, form, monkeypatch):
    """The operands of the descriptors nets.GcrnPlan records for a synthetic GCRN are what the packing functions make of
    the state dict's natural weights in the order the case builder passes them.  GcrnPlan calls the same functions: this
    pins the choice of keys and the argument order, not the packers."""
    nets, L, P = pkg("nets"), pkg("_lib"), pkg("packing")
    sd = weights("GCRN")
    monkeypatch.setattr(nets.GcrnPlan, "fused_glstm", form != "generic")
    monkeypatch.setattr(nets.GcrnPlan, "persist_lstm", form == "persistent")
    ctx = nets.Ctx("cpu")
    net = nets.GcrnPlan(ctx, sd, 1, 6, exclusive=True)
    net.build()
    mem = emu.Mem(ctx.all_tensors())
    w = lambda k: P._np(sd["glstm." + k])                            # noqa: E731
    per = lambda key: [w(key % g) for g in range(2)]                # noqa: E731
    nat = (per("lstm_list1.%d.weight_hh_l0"), per("lstm_list2.%d.weight_ih_l0"), per("lstm_list2.%d.bias_ih_l0"),
           per("lstm_list2.%d.bias_hh_l0"), per("lstm_list2.%d.weight_hh_l0"), w("ln1.weight"), w("ln1.bias"))

    def same(d, fields):
        for key, a in fields.items():
            want = np.ascontiguousarray(a, np.float32)
            assert np.asarray(mem.arr(getattr(d, key), want.size)).tobytes() == want.tobytes(), key

    if form == "generic":
        descs = [d for d, _ in net.descs if isinstance(d, L.LstmDesc)]
        assert len(descs) == 2
        for d, layer in zip(descs, ("lstm_list1", "lstm_list2")):
            same(d, dict(whh=P.pack_lstm_whh(per(layer + ".%d.weight_hh_l0"))))
    else:
        typ, pack = (L.GlstmDesc, P.pack_glstm_wavefront) if form == "wavefront" else (L.GlstmpDesc, P.pack_glstm_persistent)
        descs = [d for d, _ in net.descs if isinstance(d, typ)]
        assert len(descs) == 1
        same(descs[0], pack(*nat))
