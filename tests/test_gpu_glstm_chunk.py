"""The chunked form of the grouped-LSTM wavefront (pdse_glstm_desc.tc >= 1; csrc/lstm.hip: glstm_wave_kernel<NS, true> with
stages A and C per step, glstm_proj_kernel per chunk) launched alone through the C ABI, as tests/test_gpu_lstm_ops.py launches
the three-stage form, with natural parameters from tests/helpers/lstm_cases.py and the case table of
tests/helpers/glstm_chunk.py (shapes and regimes: see there).

Tolerance - the project's rule, unchanged (lstm_cases.check): against the float64 statement of tests/helpers/lstm_refs.py,
rel_l2 <= max(4 e32, 2e-6) and element by element max(8 m32, 2e-6), e32 and m32 from the fp32 CPU statement, never from a
kernel.  Measured: profiles/glstm_chunk_margins.txt.

Structure, bit for bit: layer 1 is the same code in the same order, so h1 of the last two frames (all the three-stage
form keeps) equals the ring's; NaN in the padded items of gx1 and a NaN-filled scratch (unused ring slots included - every
case starts from one) reach no own item; a second launch on the dirty rings and a shorter T behind a longer one; slices 1
against 2.  Refusals: tc < 1, a null ring pointer, a lag that disagrees with tc."""
import pytest
import torch

from conftest import pkg
from helpers import glstm_chunk as K
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
        pytest.exit("device error after a glstm launch: %s" % e, returncode=3)


def _launch(L, b):
    L.launch(b.desc)
    _sync()
    return b


def _run(L, case, **kw):
    return _launch(L, K.build(case, DEV, **kw))


@pytest.mark.parametrize("case", K.CASES, ids=G.by_id(K.CASES))
def test_chunked_against_float64(L, case):
    b = _run(L, case)
    G.check(case["id"], G.read(b), G.ref(case, F64), G.ref(case, F32), case["regime"])


@pytest.mark.parametrize("case", K.CASES, ids=G.by_id(K.CASES))
def test_h1_is_bit_identical_to_the_three_stage_wavefront(L, case):
    chunk = _run(L, case)
    three = _launch(L, G.build(case, DEV))                # the same case, tc == 0
    T = case["T"]
    for t in range(max(0, T - 2), T):
        assert G.same_bits(K.ring_h1(chunk, t), K.pingpong_h1(three, t)), t


STRUCT = ["glstm_s1_B3_T9_n01_cat_tc4", "glstm_s2_B33_T6_flat_il_tc4", "glstm_s2_B2_T5_flat_cat_tc4", "glstm_s1_B2_T3_offset_il_tc4"]


@pytest.mark.parametrize("name", STRUCT)
def test_nan_in_the_padding(L, name):
    """Items b >= B of gx1 hold NaN (and every ring slot, used or not, starts as NaN): the own items' outputs are finite
    (G.read) and the bits of the launch with zeros."""
    case = K.find(name)
    assert G.same_bits(G.read(_run(L, case, pad_nan=True)), G.read(_run(L, case)))


@pytest.mark.parametrize("name", STRUCT)
def test_dirty_buffers(L, name):
    """A second launch on the same, now dirty, rings; then a shorter T on the scratch the longer one left behind."""
    case = K.find(name)
    b = _run(L, case)
    first = G.read(b)
    b.out.fill_(float("nan"))
    assert G.same_bits(G.read(_launch(L, b)), first)
    short = G.variant(case, T=max(1, case["T"] - 2))
    assert G.same_bits(G.read(_run(L, short, scr=b.scr)), G.read(_run(L, short)))


@pytest.mark.parametrize("name", ["glstm_s1_B3_T9_n01_cat_tc4", "glstm_s2_B33_T6_flat_il_tc4"])
def test_slices_are_bit_identical(L, name):
    case = K.find(name)
    assert G.same_bits(G.read(_run(L, G.variant(case, slices=1))), G.read(_run(L, G.variant(case, slices=2))))


def _set(**kw):
    return lambda d: [setattr(d, k, v) for k, v in kw.items()]


REFUSALS = [
    ("tc_negative", _set(tc=-1, lag=0), "glstm: chunked form needs tc >= 1"),
    ("tc0_with_lag", _set(tc=0, lag=5), "glstm: chunked form needs tc >= 1"),
    ("lag_is_tc", _set(lag=4), "glstm: lag must be tc \\+ 1"),
    ("lag_of_three_stage", _set(lag=2), "glstm: lag must be tc \\+ 1"),
    ("null_h1_ring", _set(hT1=None), "glstm: null pointer"),
    ("null_gx2_ring", _set(gx2=None), "glstm: null pointer"),
    ("null_part_ring", _set(part=None), "glstm: null pointer"),
]


@pytest.mark.parametrize("name,mutate,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(L, name, mutate, message):
    """The descriptor raises PdseError with the message in the source and launches nothing: the NaN-filled output stays as
    it was."""
    b = K.build(K.find("glstm_s1_B3_T4_n01_il_tc4"), DEV)
    mutate(b.desc)
    with pytest.raises(L.PdseError, match=message):
        L.launch(b.desc)
    _sync()
    assert G.untouched(b), "%s: a refused descriptor launched" % name
