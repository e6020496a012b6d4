"""Operator-level parity of the TCM residual-block kernels through the C-ABI: csrc/tcm.hip (pdse_tcm_f32), csrc/tcm2.hip
tcm2_kernel (pdse_tcm2_bf16x3: modes 0 and 1, plane counts 1 / 2 / 3) and tcm2s_kernel (pdse_tcm2_stack_bf16x3), every
kernel alone against a plain float64 statement of the block (tests/helpers/tcm_refs.py, held to torch.nn's own modules
by tests/test_tcm_refs_host.py) with parameters chosen to break it: slopes from {-0.5, 0, 1, 1.7}, BatchNorm scales of
mixed sign with exact zeros, O(1) shifts and biases, saturated mask logits, weight groups at 2^-10 / 1 / 2^6, T below a
tile and below the dilation, every K-block rotation, frames tables at 0 / 1 / clamped values.  The case table and the
descriptor builder live in tests/helpers/tcm_cases.py and are replayed on the CPU emulator by the host file.

Tolerance, csrc/tcm.hip and np = 2 / 3 - the project's rule, unchanged: with e32 = rel_l2(the same statement in fp32 on
the CPU, float64), rel_l2(kernel, float64) <= max(4 * e32, 2e-6), for x_out, h_out and both branches of hs_out after
packing.tcm2_join_h, over the utterances' own frames.
np = 1 (plain bf16): rel_l2(kernel, bf16-rounding float64 reference) <= max(4 * e32, e_b / 16) for x_out, with e_b =
rel_l2(rounding reference, unrounded reference) and e32 between the fp32 and the float64 rounding references; hs_out
element by element, |value - unrounded float64 transform of the chained conv1 on the kernel's own input| <=
2^-8 |ref| + the absolute allowance of the fp32 rule (tcm_cases.check_hs_bf16).  Measured: profiles/tcm_ops_margins.txt.
Single launches at np = 1 sit at 0.27 of e_b / 16 at the worst (tcm2np1_T161_d2).  The three-block stack tcm2snp1_T161_B2
lands ABOVE e_b / 16 (4.6e-4 against 2.7e-4, e_b 4.4e-3) from flips alone - a flipped element of hs feeds the next two
blocks - and the fp32 rounding reference does the same (e32 1.6e-4), so the case passes on 4 * e32; the divisor stays 16.

Structural checks in every case (tcm_cases.read_f / read_hs): outputs sit in NaN-filled allocations, every addressed
element is finite afterwards and the margins are NaN bit for bit; hs tensors keep zero margins inside a NaN-pattern
allocation, own frames pre-filled with the pattern are all overwritten; with a frames table hs_out is zero bits from
frames[b] on.  Neither kernel masks by multiplication: NaN is the sentinel everywhere.

Deliberately not here: the stack kernel's give-up path (status != 0) - reaching it means making workgroups wait on a
counter nobody publishes; values beyond the f16x2 window (tests/test_gpu_f16x2.py)."""
import pytest
import torch

from conftest import pkg
from helpers import tcm_cases as G

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
        pytest.exit("device error after a tcm launch: %s" % e, returncode=3)


def _run(L, case):
    b = G.build(case, DEV)
    L.launch(b.desc)
    _sync()
    return b


def _check_hs(case, b, got, ref64, ref32, x_in, p_next):
    """Both branches of hs_out; the zero tail behind an utterance's own frames."""
    if b.frames:
        assert G.zero_tail(got[0], b.frames) and G.zero_tail(got[1], b.frames), "hs_out not zero from frames[b] on"
    if case["np"] == 1:
        G.check_hs_bf16(case["id"], got, x_in, p_next, b.frames)
    else:
        G.check_fp32(case["id"] + " hs_out main", got[0], ref64["vm_next"], ref32["vm_next"], b.frames)
        G.check_fp32(case["id"] + " hs_out mask", got[1], ref64["vk_next"], ref32["vk_next"], b.frames)


@pytest.mark.parametrize("case", G.TCM, ids=G.by_id(G.TCM))
def test_tcm(L, case):
    b = _run(L, case)
    B, T = case["B"], case["T"]
    ref64, ref32 = b.ref(F64), b.ref(F32)
    G.check_fp32(case["id"] + " x_out", G.read_f(b.xobuf, (B, 256, T)), ref64["x_out"], ref32["x_out"], b.frames)
    if case["chained"]:
        G.check_fp32(case["id"] + " h_out", G.read_f(b.hobuf, (B, 64, T)), ref64["h_out"], ref32["h_out"], b.frames)
    else:
        assert G.untouched_f(b.hobuf)
    assert G.read_f(b.hbuf, (B, 64, T)).equal(b.h)                   # the input stays as it was


def _tcm2(L, case):
    b = _run(L, case)
    B, T, npl = case["B"], case["T"], case["np"]
    rnd = npl == 1
    ref64, ref32 = b.ref(F64, rnd), b.ref(F32, rnd)
    x_in = b.x
    if case["mode"] == 0:
        x_in = G.read_f(b.xobuf, (B, 256, T))
        if rnd:
            G.check_bf16(case["id"] + " x_out", x_in, ref64["x_out"], ref32["x_out"], b.ref(F64)["x_out"], b.frames)
        else:
            G.check_fp32(case["id"] + " x_out", x_in, ref64["x_out"], ref32["x_out"], b.frames)
        assert G.read_hs(b.hsbuf[0], B, T, npl)[0].equal(b.v_in[0])  # hs, its margins and its surroundings stay as they were
    else:
        assert G.read_f(b.xbuf, (B, 256, T)).equal(b.x) and G.untouched_f(b.xobuf)
    if case["mode"] == 1 or case["chained"]:
        _check_hs(case, b, G.read_hs(b.hs_out, B, T, npl), ref64, ref32, x_in, b.params[0 if case["mode"] == 1 else 1])
    else:
        assert G.untouched_hs(b.hsbuf[1], pkg("packing").tcm2_hs_shape(B, T, npl))


@pytest.mark.parametrize("case", G.TCM2[3], ids=G.by_id(G.TCM2[3]))
def test_tcm2_bf16x3(L, case):
    _tcm2(L, case)


@pytest.mark.parametrize("case", G.TCM2[2], ids=G.by_id(G.TCM2[2]))
def test_tcm2_f16x2(L, case):
    _tcm2(L, case)


@pytest.mark.parametrize("case", G.TCM2[1], ids=G.by_id(G.TCM2[1]))
def test_tcm2_bf16(L, case):
    _tcm2(L, case)


@pytest.mark.parametrize("case", [c for n in (3, 2, 1) for c in G.TCM2S[n]], ids=[i for n in (3, 2, 1) for i in G.by_id(G.TCM2S[n])])
def test_tcm2_stack(L, case):
    """Three blocks, dilations (1, 32, 2), as one persistent launch, held to the composition of three references."""
    b = _run(L, case)
    B, T, npl = case["B"], case["T"], case["np"]
    rnd = npl == 1
    assert int(b.status.cpu()[0]) == 0, "a workgroup gave up waiting"
    assert bool((b.flags.cpu() == len(case["dils"])).all()), "progress counters: every tile publishes every block"
    ref64, ref32 = b.ref(F64, rnd), b.ref(F32, rnd)
    plain = b.ref(F64) if rnd else None
    for name, buf, i in (("x_out[1]", b.x_prev, -2), ("x_out[2]", b.x_last, -1)):
        got = G.read_f(buf, (B, 256, T))
        if rnd:
            G.check_bf16("%s %s" % (case["id"], name), got, ref64[i]["x_out"], ref32[i]["x_out"], plain[i]["x_out"], b.frames)
        else:
            G.check_fp32("%s %s" % (case["id"], name), got, ref64[i]["x_out"], ref32[i]["x_out"], b.frames)
    _check_hs(case, b, G.read_hs(b.hs_out, B, T, npl), ref64[-1], ref32[-1], G.read_f(b.x_last, (B, 256, T)), b.params[-1])


# ------------------------------------------------------------------ refusals
def _null(*names):
    return lambda d, b: [setattr(d, n, None) for n in names]


def _set(**kw):
    return lambda d, b: [setattr(d, k, v) for k, v in kw.items()]


TCM_REFUSALS = [
    ("null_x", _null("x"), "tcm: null pointer"), ("null_wc2", _null("wc2"), "tcm: null pointer"), ("null_xf2", _null("xf2"), "tcm: null pointer"),
    ("h_out_without_wn1", _null("wn1"), "tcm: the chained conv1 needs its weights and bias"),
    ("h_out_without_bn1", _null("bn1"), "tcm: the chained conv1 needs its weights and bias"),
    ("h_out_is_h", lambda d, b: setattr(d, "h_out", d.h), "tcm: h_out must not alias h"),
    ("T0", _set(T=0), "tcm: bad sizes"), ("dil0", _set(dil=0), "tcm: bad sizes"),
]
TCM2_REFUSALS = [
    # (name, case, mutation, message)
    ("dil0", "tcm2np3_T77_d3", _set(dil=0), r"tcm2: bad sizes \(dilation <= 32\)"),
    ("dil33", "tcm2np3_T77_d3", _set(dil=33), r"tcm2: bad sizes \(dilation <= 32\)"),
    ("mode2", "tcm2np3_T77_d3", _set(mode=2), "tcm2: mode is 0"),
    ("np4", "tcm2np3_T77_d3", _set(np=4), "tcm2: np is 3"),
    ("qexp41", "tcm2np2_T77_d3", lambda d, b: d.qexp.__setitem__(1, 41), "tcm2: qexp out of range"),
    ("qexp-41", "tcm2np2_T77_d3", lambda d, b: d.qexp.__setitem__(2, -41), "tcm2: qexp out of range"),
    ("mode1_without_hs_out", "tcm2np3_mode1_T33", _null("hs_out"), "tcm2: mode 1 writes hs_out"),
    ("hs_out_without_wn1", "tcm2np3_T77_d3", _null("wn1"), "tcm2: the chained conv1 needs its weights"),
    ("hs_out_is_hs", "tcm2np3_T77_d3", lambda d, b: setattr(d, "hs_out", d.hs), "tcm2: hs_out must not alias hs"),
    ("mode0_without_hs", "tcm2np3_T77_d3", _null("hs"), "tcm2: null pointer"),
    ("mode0_without_x_out", "tcm2np3_T77_d3", _null("x_out"), "tcm2: null pointer"),
    ("mode0_without_wbr", "tcm2np3_T77_d3", _null("wbr"), "tcm2: null pointer"),
    ("mode0_without_wc2", "tcm2np3_T77_d3", _null("wc2"), "tcm2: null pointer"),
    ("null_x", "tcm2np3_T77_d3", _null("x"), "tcm2: null pointer"),
    ("null_par", "tcm2np1_T77_d3", _null("par"), "tcm2: null pointer"),
]


def _blk(i, **kw):
    return lambda d, b: [setattr(d.blk[i], k, v) for k, v in kw.items()]


TCM2S_REFUSALS = [
    ("n0", _set(n=0), r"tcm2s: 1 \.\. PDSE_TCM2S_MAX blocks"),
    ("n_max_plus_1", lambda d, b: setattr(d, "n", pkg("_lib").TCM2S_MAX + 1), r"tcm2s: 1 \.\. PDSE_TCM2S_MAX blocks"),
    ("null_flags", _null("flags"), "tcm2s: null pointer"), ("null_status", _null("status"), "tcm2s: null pointer"),
    ("other_B", _blk(1, B=1), "tcm2s: blocks of one stack share B, T and the plane count"),
    ("other_T", _blk(2, T=32), "tcm2s: blocks of one stack share B, T and the plane count"),
    ("other_np", _blk(1, np=2), "tcm2s: blocks of one stack share B, T and the plane count"),
    ("mode1_block", _blk(1, mode=1), "tcm2s: residual blocks only"),
    ("dil33", _blk(2, dil=33), "tcm2s: dilation <= 32"),
    ("hs_not_predecessors", lambda d, b: setattr(d.blk[1], "hs", G.hptr(b.spare)), "tcm2s: block i reads the hs that block i - 1 wrote"),
    ("hs_do_not_alternate", lambda d, b: setattr(d.blk[1], "hs_out", G.hptr(b.spare)), "tcm2s: the hs buffers must alternate strictly"),
    ("x_is_x_out", lambda d, b: setattr(d.blk[0], "x_out", d.blk[0].x), "tcm2s: x and x_out of a block differ"),
    ("two_frames_tables", lambda d, b: setattr(d.blk[2], "frames", b.other_frames.data_ptr()), "tcm2s: the blocks of one stack share one frames table"),
]


def test_refusals(L):
    """Each descriptor must raise PdseError with the message in the source and launch nothing: the NaN-filled outputs stay as
    they were."""
    for name, mutate, message in TCM_REFUSALS:
        b = G.build(G.find("tcm_T33_d1"), DEV)
        mutate(b.desc, b)
        with pytest.raises(L.PdseError, match=message):
            L.launch(b.desc)
        _sync()
        assert G.untouched_f(b.xobuf) and G.untouched_f(b.hobuf), "tcm %s: a refused descriptor launched" % name
    for name, cid, mutate, message in TCM2_REFUSALS:
        b = G.build(G.find(cid), DEV)
        mutate(b.desc, b)
        with pytest.raises(L.PdseError, match=message):
            L.launch(b.desc)
        _sync()
        shape = pkg("packing").tcm2_hs_shape(b.case["B"], b.case["T"], b.case["np"])
        assert G.untouched_f(b.xobuf) and G.untouched_hs(b.hsbuf[0 if b.case["mode"] == 1 else 1], shape), "tcm2 %s: a refused descriptor launched" % name
    for name, mutate, message in TCM2S_REFUSALS:
        b = G.build(G.find("tcm2snp3_frames_64_41_T_T161"), DEV)
        shape = pkg("packing").tcm2_hs_shape(b.case["B"], b.case["T"], 3)
        b.spare = G._hsbuf(None, shape, DEV)
        b.other_frames = torch.tensor([161, 161, 161], dtype=torch.int32, device=DEV)
        mutate(b.desc, b)
        with pytest.raises(L.PdseError, match=message):
            L.launch(b.desc)
        _sync()
        assert G.untouched_f(b.xobuf) and G.untouched_hs(b.hsbuf[1], shape) and G.untouched_hs(b.spare, shape), "tcm2s %s: a refused descriptor launched" % name
        assert bool((b.flags.cpu() == -1).all()) and int(b.status.cpu()[0]) == 0
