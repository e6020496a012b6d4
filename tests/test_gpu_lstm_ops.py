"""Operator-level parity of the recurrent core of the GCRN prior through the C-ABI: csrc/lstm.hip lstm_step_kernel
(pdse_lstm_f32) and glstm_wave_kernel<1|2> (pdse_glstm_f32), csrc/lstmp.hip glstm_persist_kernel<1|2|4|8>
(pdse_glstm_persistent_f32) and csrc/misc.hip ln_kernel (pdse_layernorm_f32), every kernel alone against a plain float64
statement of the grouped LSTM in natural parameters (tests/helpers/lstm_refs.py, held to torch.nn.LSTM / LayerNorm by
tests/test_lstm_refs_host.py), packed through the product's own packing (packing.pack_lstm_whh, pack_glstm_wavefront,
pack_glstm_persistent).  The case table and the descriptor builder live in tests/helpers/lstm_cases.py and are replayed
on the CPU emulator by the host file.  Regimes n01 / hot / sat / tiny / offset / flat: see lstm_cases.

Tolerance - the project's rule, unchanged, over own items: with e32 = rel_l2(the same statement in fp32 on the CPU,
float64), rel_l2(kernel, float64) <= max(4 * e32, 2e-6); and element by element max |kernel - float64| <=
max(8 * max |fp32 - float64|, 2e-6) (lstm_cases.check).  Both measured against the fp32 CPU statement, never against
another kernel form.  Regime tiny is judged by the element bound alone.  Measured: profiles/lstm_ops_margins.txt.

What the offset and flat regimes found in both fused forms (figures in the margins file): with LayerNorm 1's moments as
E[x^2] - mu^2 and the fold as rs (W' y - mu W' 1), glstmp_B8_T7_flat_cat sat at 26 times the rel_l2 bound (7.5e-4 against
2.9e-5) and glstm_s2_B32_T33_flat_il at 5.6 times; the offset cases at 1.2 to 2.4 times.  Both forms now carry the second
moment as a sum of squared deviations (Chan's combine, fixed order) and multiply W' by y - k, k the item's own first
feature, so that neither the variance nor the projection is a difference of two numbers of the size of the mean.

Structural checks in every case (lstm_cases.read): y sits in a NaN-filled allocation with margins and gaps between its
frames and items, every addressed element is finite afterwards and everything else NaN bit for bit; all scratch and the
granule buffer hold NaN before the launch; status is zero after every persistent launch.  Per kernel: NaN in the padded
rows b >= B of gx / gx1, a second launch on the same buffers, a shorter T behind a longer one on the same scratch, item
B - 1 alone (across granule widths for the persistent form: B = 3 and B = 8 against B = 1), slices 1 against 2 - all
bit for bit; both y layouts; refusals.

Deliberately not here: the persistent kernel's give-up path (status != 0) - reaching it means a launch whose 256
workgroups cannot all be resident, or that waits on granules nobody publishes; no launch here is constructed that could
reach it (B <= 8, T <= 160, one launch at a time, synchronised before the next).  The LayerNorm has no padded rows and no
scratch: of the structural checks only the second launch applies to it."""
import pytest
import torch

from conftest import pkg
from helpers import lstm_cases as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64


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
        pytest.exit("device error after an lstm launch: %s" % e, returncode=3)


def _launch(L, b):
    L.launch(b.desc)
    _sync()
    if b.case["kernel"] == "glstmp":
        assert int(b.status.cpu()[0]) == 0, "a workgroup gave up waiting"
    return b


def _run(L, case, **kw):
    return _launch(L, G.build(case, DEV, **kw))


def _parity(L, case):
    b = _run(L, case)
    G.check(case["id"], G.read(b), G.ref(case, F64), G.ref(case, F32), case.get("regime", "n01"))


@pytest.mark.parametrize("case", G.LSTM, ids=G.by_id(G.LSTM))
def test_lstm(L, case):
    _parity(L, case)


@pytest.mark.parametrize("case", G.GLSTM, ids=G.by_id(G.GLSTM))
def test_glstm(L, case):
    _parity(L, case)


@pytest.mark.parametrize("case", G.GLSTMP, ids=G.by_id(G.GLSTMP))
def test_glstm_persistent(L, case):
    _parity(L, case)


@pytest.mark.parametrize("case", G.LN, ids=G.by_id(G.LN))
def test_layernorm(L, case):
    b = _run(L, case)
    first, at = G.read(b), b.pos.reshape(-1)
    G.check(case["id"], first.reshape(-1), G.ref(case, F64)[at], G.ref(case, F32)[at])
    assert G.same_bits(G.read(_launch(L, b)), first)    # once more onto its own output


# ------------------------------------------------------------------ structure, bit for bit
STRUCT = ["lstm_B31_T7_tiny_cat", "lstm_B33_T7_n01_cat", "glstm_s1_B31_T3_sat_il", "glstm_s2_B33_T7_n01_cat",
          "glstmp_B3_T3_sat_cat", "glstmp_B3_Bp3_T7_n01_il", "glstmp_B8_T7_flat_cat"]


@pytest.mark.parametrize("name", [n for n in STRUCT if "Bp3" not in n])
def test_nan_in_the_padding(L, name):
    """Rows b >= B of gx / gx1 hold NaN: the own items' outputs are finite (G.read) and the bits of the launch with zeros."""
    case = G.find(name)
    assert G.same_bits(G.read(_run(L, case, pad_nan=True)), G.read(_run(L, case)))


@pytest.mark.parametrize("name", STRUCT)
def test_dirty_buffers(L, name):
    """A second launch on the same, now dirty, scratch; then a shorter T on the scratch the longer one left behind."""
    case = G.find(name)
    b = _run(L, case)
    first = G.read(b)
    b.out.fill_(float("nan"))
    assert G.same_bits(G.read(_launch(L, b)), first)
    short = G.variant(case, T=max(1, case["T"] - 2))
    assert G.same_bits(G.read(_run(L, short, scr=b.scr)), G.read(_run(L, short)))


@pytest.mark.parametrize("name", STRUCT + ["glstmp_B8_T33_hot_cat", "glstmp_B2_T7_offset_cat", "glstm_s1_B32_T7_offset_cat"])
def test_last_item_alone(L, name):
    """Item B - 1 of the batch, run alone (B = 1: another batch tile count, another granule width), is bit-identical."""
    case = G.find(name)
    B = case["B"]
    whole = G.read(_run(L, case))
    alone = G.read(_run(L, G.variant(case, B=1, first_item=B - 1, Bp=32 if case["Bp"] >= 32 else case["Bp"])))
    assert G.same_bits(alone[:, 0], whole[:, B - 1])


@pytest.mark.parametrize("name", ["glstm_s2_B33_T7_n01_cat", "glstm_s1_B32_T7_offset_cat", "glstm_s2_B32_T33_flat_il"])
def test_slices_are_bit_identical(L, name):
    case = G.find(name)
    assert G.same_bits(G.read(_run(L, G.variant(case, slices=1))), G.read(_run(L, G.variant(case, slices=2))))


# ------------------------------------------------------------------ refusals
def _set(**kw):
    return lambda d: [setattr(d, k, v) for k, v in kw.items()]


REFUSALS = [
    ("lstm_B1_T1_n01_il", "H256", _set(H=256), "lstm: bad sizes"),
    ("lstm_B1_T1_n01_il", "Bp48", _set(Bp=48), "lstm: bad sizes"),
    ("lstm_B33_T1_hot_il", "Bp_below_B", _set(Bp=32), "lstm: bad sizes"),
    ("glstm_s1_B1_T1_n01_cat", "G1", _set(G=1), "glstm: bad sizes"),
    ("glstm_s1_B1_T1_n01_cat", "slices3", _set(slices=3), "glstm: slices is 0 / 1"),
    ("glstm_s1_B1_T1_n01_cat", "grid_z", _set(Bp=32 * 21846), "glstm: bad sizes"),          # (Bp / 32) * 3 = 65538 > 65535
    ("glstmp_B1_T1_n01_cat", "gran_unaligned", lambda d: setattr(d, "gran", d.gran + 8), "glstmp: granule buffer must be 16-byte aligned"),
    ("glstmp_B1_T1_n01_cat", "T0", _set(T=0), "glstmp: bad sizes"),
    ("ln_B1_T3_N1024_r4_blk0_n01", "N1025", _set(N=1025), "layernorm: bad sizes"),
    ("ln_B1_T3_N1024_r4_blk0_n01", "r0", _set(r=0), "layernorm: bad sizes"),
    ("ln_B1_T3_N1024_r4_blk0_n01", "blk4", _set(blk=4), "layernorm: blk is 0 or 8"),
]


@pytest.mark.parametrize("cid,name,mutate,message", REFUSALS, ids=["%s_%s" % (r[0].split("_")[0], r[1]) for r in REFUSALS])
def test_refusals(L, cid, name, mutate, message):
    """The descriptor raises PdseError with the message in the source and launches nothing: the NaN-filled output stays as
    it was."""
    b = G.build(G.find(cid), DEV)
    mutate(b.desc)
    with pytest.raises(L.PdseError, match=message):
        L.launch(b.desc)
    _sync()
    assert G.untouched(b), "%s: a refused descriptor launched" % name
