"""The chunked form of the grouped-LSTM wavefront without a GPU: the numpy restatement of its launch sequence, ring indexing,
lag and LayerNorm fold (tests/helpers/glstm_chunk.py: run_chunk) on the case table the GPU file runs, held to the float64
statement (tests/helpers/lstm_refs.py) by the project's rule, unchanged (lstm_cases.check: rel_l2 <= max(4 e32, 2e-6),
element bound max(8 m32, 2e-6), e32 / m32 from the fp32 CPU statement); the launch sequence itself; and the packer the form
shares with the three-stage wavefront (packing.pack_glstm_wavefront) as a pure function."""
import numpy as np
import pytest
import torch

import emu
from conftest import pkg
from helpers import glstm_chunk as K
from helpers import lstm_cases as G

F32, F64 = torch.float32, torch.float64


def _replay(case, **kw):
    b = K.build(case, "cpu", **kw)
    with np.errstate(over="ignore", invalid="ignore"):
        K.run_chunk(b.desc, emu.Mem(G.tensors(b)))
    return b


@pytest.mark.parametrize("case", K.CASES, ids=G.by_id(K.CASES))
def test_restatement_against_float64(case):
    b = _replay(case)
    G.check(case["id"], G.read(b), G.ref(case, F64), G.ref(case, F32), case["regime"])


def test_case_table_reaches_what_it_names():
    shapes = {(c["B"], c["T"], c["tc"]) for c in K.CASES}
    assert shapes == set(K.SHAPES) and len(K.CASES) == len(K.SHAPES) * 3
    for B, T, tc in K.SHAPES:
        assert {c["regime"] for c in K.CASES if (c["B"], c["T"], c["tc"]) == (B, T, tc)} == {"n01", "offset", "flat"}
    assert {c["slices"] for c in K.CASES} == {1, 2} and {c["layout"] for c in K.CASES} == {"il", "cat"}
    assert any(c["Bp"] == 64 and c["B"] % 32 for c in K.CASES)


@pytest.mark.parametrize("T,tc", [(1, 4), (3, 4), (4, 4), (5, 4), (9, 4), (33, 32), (401, 32), (7, 1)])
def test_launch_sequence(T, tc):
    """T + tc + 1 steps (less the steps of T < lag that have neither stage) and ceil(T / tc) projections; every frame is
    projected exactly once, after layer 1 wrote it and before layer 2 reads it; a ring slot is not rewritten while a later
    launch still reads what it held."""
    seq = K.launches(T, tc)
    lag, R = tc + 1, 2 * tc
    steps = [op[1] for op in seq if op[0] == "step"]
    projs = [op for op in seq if op[0] == "proj"]
    assert len(projs) == -(-T // tc) and steps == [s for s in range(T + tc + 1) if s < T or s >= lag]
    assert sorted(t for _, t0, nf in projs for t in range(t0, t0 + nf)) == list(range(T))
    assert all(nf <= tc and t0 % tc == 0 for _, t0, nf in projs)
    h1_slot, gx_slot = {}, {}                             # slot -> frame it holds
    done_a, done_p = set(), set()
    for op in seq:
        if op[0] == "proj":
            for t in range(op[1], op[1] + op[2]):
                assert t in done_a and h1_slot[(t + 1) % R] == t
                gx_slot[t % R] = t
                done_p.add(t)
            continue
        s = op[1]
        if s < T:
            assert s == 0 or h1_slot[s % R] == s - 1
            old = h1_slot.get((s + 1) % R)
            assert old is None or old in done_p          # nobody still needs the frame this store replaces
            h1_slot[(s + 1) % R] = s
            done_a.add(s)
        t = s - lag
        if 0 <= t < T:
            assert t in done_p and gx_slot[t % R] == t


def test_nan_in_the_padding_and_dirty_scratch_on_the_restatement():
    case = K.find("glstm_s2_B33_T6_flat_il_tc4")
    b = _replay(case)
    assert G.same_bits(G.read(_replay(case, pad_nan=True)), G.read(b))
    short = G.variant(case, T=4)
    assert G.same_bits(G.read(_replay(short, scr=b.scr)), G.read(_replay(short)))


def test_packer_is_a_pure_function():
    """Same input, same bytes; the input is not modified.  The chunk projection walks K in stage B's order, so both forms
    upload the one set of operands packing.pack_glstm_wavefront returns."""
    P = pkg("packing")
    p = G.natural(K.CASES[0])
    per = lambda key: [p[key % g] for g in range(G.G_)]   # noqa: E731
    nat = (per("lstm_list1.%d.weight_hh_l0"), per("lstm_list2.%d.weight_ih_l0"), per("lstm_list2.%d.bias_ih_l0"),
           per("lstm_list2.%d.bias_hh_l0"), per("lstm_list2.%d.weight_hh_l0"), p["ln1.weight"], p["ln1.bias"])
    before = [np.array(a, copy=True) for x in nat for a in (x if isinstance(x, list) else [x])]
    one, two = P.pack_glstm_wavefront(*nat), P.pack_glstm_wavefront(*nat)
    after = [a for x in nat for a in (x if isinstance(x, list) else [x])]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert set(one) == set(two) == {"whh1", "whh2", "wih2", "r2", "c2"}
    for k in one:
        assert np.asarray(one[k]).tobytes() == np.asarray(two[k]).tobytes(), k
