"""Operator-level parity of the gather-GEMM convolutions through the C-ABI (pdse_gconv_f32, epilogues LINEAR and GLU):
csrc/gconv.hip (korder 0), csrc/gconv2.hip (korder 1), csrc/gconv4.hip (korder 3 / 4 / 5) and the shared epilogue of
csrc/gconv_common.h, every kernel alone against a plain float64 statement of the operator (tests/helpers/gconv_refs.py,
held to torch's own convolutions by tests/test_gconv_refs_host.py), at the smallest shapes that reach each path: channel
and position tails, every MT instantiation with full and half-empty z-slices, partial K chunks, the large LDS ring, the
16-byte store paths and their fallbacks, the load-side features.  The case tables live in tests/helpers/gconv_cases.py
and are replayed on the CPU emulator by the host file, which also pins each case to the korder it names.

BIGLU (korder 0 / 1 / 2, the nx_* chain, the dual phase, csrc/bglu.hip) is deliberately out of scope here: it is a
test file of its own.

Tolerance, the rule of tests/test_gpu_aia_ops.py unchanged: with e32 = rel_l2(the same statement in fp32 on the CPU,
float64), rel_l2(kernel, float64) <= max(4 * e32, 2e-6).  For korder 4 both references round the weights and the
gathered activations to bf16 first; what remains is fp32 accumulation.  Measured values: profiles/gconv_ops_margins.txt.

Two structural checks in every case (gconv_cases.build / check_stores): the output is a NaN-filled buffer with margins
around and gaps inside the addressed box - exactly the addressed elements are finite afterwards, the rest is NaN bit
for bit; every input sits inside an allocation whose margins hold NaN, so a gather beyond [0,Tin) x [0,Fin) poisons the
result.  All four kernels mask out-of-range taps by selection, none by multiplication: NaN serves as the sentinel for
every one of them (no kernel needed the largest finite float instead)."""
import math

import pytest
import torch

from conftest import pkg
from helpers import gconv_cases as G

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


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault fails every later launch of the process: stop instead of piling them on
        pytest.exit("device error after a gconv launch: %s" % e, returncode=3)


def _run(L, case, korder=None, **kw):
    b = G.build(case, DEV, korder, **kw)
    assert b.desc.korder == (case["korder"] if korder is None else korder)
    L.launch(b.desc)
    _sync()
    return b, G.check_stores(b)


def _case(L, case, korder=None):
    b, got = _run(L, case, korder)
    G.check_norm(got, b.ref(torch.float64), b.ref(torch.float32))


@pytest.mark.parametrize("case", G.GENERIC, ids=G.by_id(G.GENERIC))
def test_generic(L, case):
    _case(L, case)


@pytest.mark.parametrize("case", G.K1, ids=G.by_id(G.K1))
def test_pipelined(L, case):
    _case(L, case)


@pytest.mark.parametrize("case,mt,max_mt", G.K1_WIDE, ids=[w[0]["id"] for w in G.K1_WIDE])
def test_pipelined_widened(L, case, mt, max_mt):
    """MT 2 / MT 4 (and with them the PP2 / PP4 ping-pong variants) at the smallest grid at which pick_mt widens; the
    shapes are derived from its rule (gconv_cases.widening_shape), the host file asserts them against it."""
    assert G.pick_mt(case["B"], case["Tout"] * case["Fout"], case["Cout"], max_mt) == mt
    _case(L, case)


@pytest.mark.parametrize("korder", [3, 4, 5])
@pytest.mark.parametrize("case", G.GEMM, ids=G.by_id(G.GEMM))
def test_gemm(L, case, korder):
    _case(L, case, korder)


@pytest.mark.parametrize("case", G.GEMM_WSCALE, ids=G.by_id(G.GEMM_WSCALE))
def test_gemm_f16x2_weight_exponent(L, case):
    """korder 5 with the weights scaled by 2^-10 and 2^6: wexp differs and the kernel's descaling is exercised."""
    _case(L, case, 5)


@pytest.mark.parametrize("korder", [3, 4, 5])
def test_gemm_chained_pair(L, korder):
    """A launch that writes a channel-blocked tensor (out_cr = 8) read by a launch with pdse_src.blk = 8, held to the
    composition of the two references."""
    ca, cb = G.CHAIN
    a, got_a = _run(L, ca, korder)
    G.check_norm(got_a, a.ref(torch.float64), a.ref(torch.float32))
    strides, off = a.layout
    b, got_b = _run(L, cb, korder, src=(a.buf, G.MARGIN + off, (strides[0], strides[1], strides[3], strides[4])))
    assert b.desc.in0.blk == 8
    G.check_norm(got_b, b.ref(torch.float64, a.ref(torch.float64)), b.ref(torch.float32, a.ref(torch.float32)))


# ------------------------------------------------------------------ refusals
def _find(cases, name):
    return next(c for c in cases if c["id"] == name)


def _valid_ptr(b):
    return b.keep[0].data_ptr()


REFUSALS = [
    # (name, table, case, korder, mutation of the descriptor, message in the source)
    ("odd_channels", G.GENERIC, "c6_lin_s2_cout33", None, lambda d, b: setattr(d.in0, "C", 5), "channel counts must be even"),
    ("ksteps_korder0", G.GENERIC, "c6_lin_s2_cout33", None, lambda d, b: setattr(d, "ksteps", d.ksteps + 1), r"ksteps != ntaps\*Cin/2"),
    ("cin1_two_channels", G.GENERIC, "cin1_bins5_cout33", None, lambda d, b: setattr(d.in0, "C", 2),
     "cin1 path needs exactly one input channel"),
    ("xf2_without_second_set", G.GENERIC, "xf1_lin_c6", None, lambda d, b: setattr(d, "xf_mode", 2), "xf_mode 2 without second set"),
    ("post_scale_alone", G.GENERIC, "post_lin_prelu", None, lambda d, b: setattr(d, "post_shift", None),
     "post_scale/post_shift must come together"),
    ("k1_no_instantiation", G.K1, "lin_t4_c4_cout33", None, lambda d, b: setattr(d, "ntaps", 2), "no pipelined instantiation"),
    ("k1_pad_row", G.K1, "lin_t4_c4_cout33", None, lambda d, b: setattr(d, "padrow", _valid_ptr(b)), "no pad row"),
    ("k1_ksteps_mod4", G.K1, "lin_t4_c4_cout33", None, lambda d, b: setattr(d, "ksteps", d.ksteps + 2), r"ksteps % 4 == 0"),
    ("k3_c0_8", G.GEMM, "c16_t1_lin16_p1", 3, lambda d, b: setattr(d.in0, "C", 8), "channel counts in multiples of 16"),
    ("k3_13_taps", G.GEMM, "c16_t1_lin16_p1", 3, lambda d, b: (setattr(d, "ntaps", 13), setattr(d, "ksteps", 13 * 8)), "<= 12 taps"),
    ("k3_xf", G.GEMM, "c16_t1_lin16_p1", 3,
     lambda d, b: (setattr(d, "xf_mode", 1), setattr(d, "xf_scale0", _valid_ptr(b)), setattr(d, "xf_shift0", _valid_ptr(b))),
     "no load transform"),
    ("k3_blocked_and_plain", G.GEMM, "blk_c16c48_glu32", 3, lambda d, b: setattr(d.in1, "blk", 0), "both blocked or both plain"),
    ("k3_blocked_sf", G.GEMM, "blk_c32_lin48", 3, lambda d, b: setattr(d.in0, "sf", 6), "strides in multiples of 4 floats"),
    ("k3_blocked_base", G.GEMM, "blk_c32_lin48", 3, lambda d, b: setattr(d.in0, "ptr", d.in0.ptr + 4), "16-byte aligned base"),
    ("k3_biglu", G.GEMM, "c16_t1_lin16_p1", 3, lambda d, b: setattr(d, "epi", 2), "LINEAR / GLU epilogues only"),
    ("k5_wexp_41", G.GEMM, "c16_t1_lin16_p1", 5, lambda d, b: setattr(d, "wexp", 41), "split-bf16 GEMM convolutions need"),
]


def test_refusals(L):
    """Each descriptor must raise PdseError with the message in the source and launch nothing: the NaN-filled output
    stays as it was."""
    nanbits = torch.full((1,), math.nan).view(torch.int32)
    for name, table, cid, korder, mutate, message in REFUSALS:
        b = G.build(_find(table, cid), DEV, korder)
        mutate(b.desc, b)
        with pytest.raises(L.PdseError, match=message):
            L.launch(b.desc)
        _sync()
        assert bool((b.buf.cpu().view(torch.int32) == nanbits).all()), "%s: a refused descriptor launched" % name
