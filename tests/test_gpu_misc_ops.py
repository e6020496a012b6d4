"""Operator-level parity of the kernels of csrc/misc.hip that only whole-network fixtures reached so far, every kernel alone
through the C-ABI against a plain float64 statement (tests/helpers/misc_refs.py, held to torch's own modules by
tests/test_misc_refs_host.py): gcrnlast_kernel (pdse_gcrnlast_f32), time_embed_kernel (pdse_time_embed_f32), wavprep_kernel
(pdse_wavprep_f32, dense and reflect_own), ola_kernel (pdse_ola_f32, dense and RAGGED), maskloss_* (pdse_masked_mse_f32).  The
case tables and the descriptor builder live in tests/helpers/misc_cases.py and are replayed on the CPU emulator by the host
file.

gcrnlast: the descriptor comes from packing.gcrn_last_fields (the kernel reads the packed matrix fcp alone); the skip half
spans -30 .. +5, gate logits run from O(1) to about +-40, the BatchNorm scale is positive, negative or exactly zero, the three
taps of both convolutions are independent (bins 0, 1, 159, 160 tell them apart), the Linear is dense.  B x T from one row to
16419 rows: 514 tiles on 512 workgroups, so that workgroups 0 and 1 take a second trip of the tile loop (re-using ys / xs) and
the last tile is ragged; there rows 0 .. 63 and the rows of tiles 512 and 513 are also held to the tolerance on their own, since
a stale tile is diluted in the norm of the whole tensor.

Tolerance - the project's rule, unchanged: with e32 = rel_l2(the same statement in fp32 on the CPU, float64),
rel_l2(kernel, float64) <= max(4 * e32, 2e-6) over the addressed elements (misc_cases.check); for time_embed the fp32 statement
adds the products one by one in the kernel's order; for wavprep the rule holds for xpad and for c.  Masked MSE: 2e-6 relative
to the float64 expression, the margin tests/test_gpu_valid.py states for this kernel, and two launches agree bit for bit.
Measured: profiles/misc_ops_margins.txt.

Structural checks in every case: outputs sit in NaN-filled allocations, every addressed element is finite afterwards and the
rest is NaN bit for bit (for gcrnlast that includes the other decoder's channel plane); inputs sit between NaN margins, and
frames an utterance does not own hold NaN.  wavprep: the reflected samples carry the bits of their mirror images, zeros behind
a reflected tail.  time_embed: finite steps outside the table give the bits of the clamped steps."""
import pytest
import torch

from conftest import pkg
from helpers import misc_cases as G

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
        pytest.exit("device error after a misc launch: %s" % e, returncode=3)


def _run(L, case):
    b = G.build(case, DEV)
    L.launch(b.desc)
    _sync()
    return b


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ GCRN tail
@pytest.mark.parametrize("case", G.GCRN, ids=G.by_id(G.GCRN))
def test_gcrnlast(L, case):
    b = _run(L, case)
    B, T = case["B"], case["T"]
    got = G.read_plane(b.outbuf, B, T)
    ref64, ref32 = b.ref(F64), b.ref(F32)
    G.check(case["id"], got, ref64, ref32)
    assert G.read_f(b.in0buf, (B, 16, T, 80)).equal(b.in0) and G.read_f(b.in1buf, (B, 16, T, 80)).equal(b.in1)
    if case is G.GCRN_BIG:
        rows = B * T
        assert G.gcrn_ntiles(case) > G.GCRN_GRID_CAP
        flat = [a.reshape(rows, 161) for a in (got, ref64, ref32)]
        for name, lo, hi in (("rows 0..63", 0, 64), ("tile 512", 512 * 32, 513 * 32), ("tile 513", 513 * 32, rows)):
            G.check("%s %s" % (case["id"], name), *(a[lo:hi] for a in flat))


def test_gcrnlast_refusals(L):
    for name, mutate, message in (("null_fcp", lambda d: setattr(d, "fcp", None), "gcrn_last: null pointer"),
                                  ("null_in1", lambda d: setattr(d, "in1", None), "gcrn_last: null pointer"),
                                  ("T0", lambda d: setattr(d, "T", 0), "gcrn_last: bad sizes")):
        b = G.build(G.find("gl_B3_T7"), DEV)
        mutate(b.desc)
        with pytest.raises(L.PdseError, match=message):
            L.launch(b.desc)
        _sync()
        assert G.untouched_f(b.outbuf), name


# ------------------------------------------------------------------ step embedding
@pytest.mark.parametrize("case", G.TIME, ids=G.by_id(G.TIME))
def test_time_embed(L, case):
    b = _run(L, case)
    B, NF = case["B"], case["NF"]
    (t64, o64), (t32, o32) = b.ref(F64), b.ref(F32)
    got = G.read_f(b.outbuf, (B, NF))
    if NF:
        G.check(case["id"] + " out", got, o64, o32)
    if case["temb"]:
        G.check(case["id"] + " temb", G.read_f(b.tembbuf, (B, 512)), t64, t32)
    else:
        assert G.untouched_f(b.tembbuf)


@pytest.mark.parametrize("case", G.TIME_OOR, ids=G.by_id(G.TIME_OOR))
def test_time_embed_clamps_the_table_walk(L, case):
    """t = -3.5 and max_steps + 10.25: rows 0 and max_steps - 1, as for t = 0 and t = max_steps - 1 - an unclamped walk reads the
    NaN margin of the table (or beyond)."""
    b = _run(L, case)
    w = _run(L, dict(case, t=case["clamped"]))
    B, NF = case["B"], case["NF"]
    for buf, other, shape in ((b.outbuf, w.outbuf, (B, NF)), (b.tembbuf, w.tembbuf, (B, 512))):
        assert torch.equal(_bits(G.read_f(buf, shape)), _bits(G.read_f(other, shape)))
    (t64, o64), (t32, o32) = w.ref(F64), w.ref(F32)
    G.check(case["id"] + " out", G.read_f(b.outbuf, (B, NF)), o64, o32)


def test_time_embed_refusals(L):
    for name, mutate, message in (("null_table", lambda d: setattr(d, "table", None), "time_embed: null pointer"),
                                  ("NF_without_wfT", lambda d: setattr(d, "wfT", None), "time_embed: folded weights missing"),
                                  ("max_steps0", lambda d: setattr(d, "max_steps", 0), "time_embed: bad sizes")):
        b = G.build(G.find("te_NF513_B1_ms50"), DEV)
        mutate(b.desc)
        with pytest.raises(L.PdseError, match=message):
            L.launch(b.desc)
        _sync()
        assert G.untouched_f(b.outbuf) and G.untouched_f(b.tembbuf), name


# ------------------------------------------------------------------ waveform front end
@pytest.mark.parametrize("case", G.WAVPREP, ids=G.by_id(G.WAVPREP))
def test_wavprep(L, case):
    b = _run(L, case)
    B, Ln, pad = case["B"], case["L"], case["pad"]
    got = G.read_f(b.xpadbuf, (B, Ln + 2 * pad))
    (x64, c64), (x32, c32) = b.ref(F64), b.ref(F32)
    G.check(case["id"] + " xpad", got, x64, x32)
    if case["c"]:
        c = G.read_f(b.cbuf, (B,))
        if case["normalize"]:
            G.check(case["id"] + " c", c, c64, c32)
        else:
            assert torch.equal(c, torch.ones(B))
    else:
        assert G.untouched_f(b.cbuf)
    assert G.read_f(b.wavbuf, (B, Ln)).equal(b.x)
    bits = _bits(got)
    for i in range(B):
        n = G.own_len(case, i)
        head = bits[i, :2 * pad + 1]
        assert torch.equal(head, head.flip(0)), "xpad[pad - k] != xpad[pad + k]"
        tail = bits[i, n - 1:n + 2 * pad]                        # centred on the last own sample, xpad[pad + n - 1]
        assert torch.equal(tail, tail.flip(0)), "the far end is not the mirror image of the last samples"
        assert not bits[i, n + 2 * pad:].any(), "not zero bits behind the reflected tail"
        if not case["normalize"]:
            assert torch.equal(bits[i, pad:pad + n], _bits(b.x[i, :n]))


def test_wavprep_refusals(L):
    for name, mutate, message in (("pad_is_L", lambda d: setattr(d, "pad", d.L), "wavprep: reflect padding needs pad < L"),
                                  ("null_xpad", lambda d: setattr(d, "xpad", None), "wavprep: bad descriptor")):
        b = G.build(G.find("wp_L161"), DEV)
        mutate(b.desc)
        with pytest.raises(L.PdseError, match=message):
            L.launch(b.desc)
        _sync()
        assert G.untouched_f(b.xpadbuf) and G.untouched_f(b.cbuf), name


# ------------------------------------------------------------------ overlap-add
@pytest.mark.parametrize("case", G.OLA, ids=G.by_id(G.OLA))
def test_ola(L, case):
    b = _run(L, case)
    B, Ln = case["B"], case["L"]
    got = G.read_f(b.outbuf, (B, Ln))
    G.check(case["id"], got, b.ref(F64), b.ref(F32))
    bits = _bits(got)
    if case["zero_w0"]:                                            # sample i sits at i + 4 of its frame: window index 0 at i = 4, 12, ..
        assert not bits[:, 4::8].any() and bool((got[:, 5::8] != 0).all())
    if b.lens is not None:
        for i, n in enumerate(b.lens):
            assert not bits[i, min(max(n, 0), Ln):].any()
    if b.nframes is not None:
        for i, n in enumerate(b.nframes):
            if n <= 0:
                assert not bits[i].any()


# ------------------------------------------------------------------ masked MSE
@pytest.mark.parametrize("case", G.MASKLOSS, ids=G.by_id(G.MASKLOSS))
def test_masked_mse(L, case):
    b = _run(L, case)
    n = case["shape"][0] * L.MASKLOSS_BLOCKS
    got, part = G.read_f(b.outbuf, (1,)), G.read_d(b.partial, n)
    want = b.ref()
    print("%s: loss %.9e  float64 %.9e  rel %.3e" % (case["id"], float(got[0]), want, abs(float(got[0]) - want) / want))
    assert abs(float(got[0]) - want) <= 2e-6 * want
    again = _run(L, case)
    assert torch.equal(_bits(G.read_f(again.outbuf, (1,))), _bits(got))
    assert torch.equal(G.read_d(again.partial, n).view(torch.int64), part.view(torch.int64))
    for i, f in enumerate(case["frames"]):                         # an utterance without frames adds nothing
        assert (float(part.reshape(-1, L.MASKLOSS_BLOCKS)[i].sum()) == 0.0) == (f <= 0)
