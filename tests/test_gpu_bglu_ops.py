"""Operator-level parity of the eps-net block kernels through the C-ABI: csrc/bglu.hip bglu_kernel (pdse_bglu_planes: the five
dispatched forms enc1 / enc / enc5 / dec / dec1 at plane counts 3 / 2 / 1, 15 instantiations) and planes_conv_kernel
(pdse_split_planes with weights), every launch alone against a plain float64 statement of the stage
(tests/helpers/bglu_refs.py, held to torch.nn's own modules by tests/test_bglu_refs_host.py) with parameters chosen to break
it: PReLU slopes from {-0.5, 0, 0.25, 1}, BatchNorm scales of mixed sign with exact zeros and variances down to 1e-3, O(1)
shifts and biases, saturated gates (l_conv / r_conv biases of +-30), the four weight groups at 2^-10 / 1 / 2^6, per-item and
constant biases, the frame-0 biases of stage 1, odd and even bin counts under the parity split.  The case table, the
descriptor builder and the checks live in tests/helpers/bglu_cases.py and are replayed on the CPU emulator by the host file.

Geometry: for every form and plane count one partial tile at T = 1 (seven idle waves; frame 0 the only frame), several tiles
with neither P a multiple of 32 nor the tiles of 8, three rounds over two workgroups per item (B = 128: trip counts 2 and 1,
a last round of two tiles, the prefetch of the next round's positions), and B = 1.

Tolerance, np = 3 / 2 - the project's rule, unchanged: with e32 = rel_l2(the same statement in fp32 on the CPU, float64),
rel_l2(kernel, float64) <= max(4 * e32, 2e-6) for every output tensor (nx_hp through packing.hp_join, the skip tensors
through their [B + 1][8][T][F][4] parity-split layout, out through its strides).
np = 1 (plain bf16), fp32 outputs: rel_l2(kernel, bf16-rounding float64 reference) <= max(4 * e32r, e_b / D) with e_b =
rel_l2(rounding reference, unrounded reference) and e32r between the fp32 and the float64 rounding references; the plane
output element by element, |value - ref| <= 2^-8 |ref| + the absolute allowance of the fp32 rule (tcm_cases.check_elems_bf16),
ref being the float64 chained conv1 of the rounding reference (bf16 weights on the REFERENCE's bf16-rounded Y, the result itself
left unrounded): the kernel's own Y never reaches memory, so a
rounding of Y (or of G before it) that the kernel's fp32 arithmetic carried across a tie is inside what the element rule
absorbs here, where the TCM tests could hand the kernel's own input to the reference.
D = 8 (bglu_cases.DIV), from the measurements in profiles/bglu_ops_margins.txt by the rule "the largest power of two at which the
worst case sits at or below half its bound, never below 4": started from the TCM tests' 16, every fp32 output at np = 1 lies
below 0.02 e_b except enc5np1_tiles_B2_T9_F40 at 0.054 e_b (2.0e-4 against e_b 3.7e-3) - 0.86 of e_b / 16, 0.43 of e_b / 8.  That
case (hostile parameters, conv2 at 2^-10, BatchNorm shifts that cancel most of conv2's output) is also the one with the largest
error at np = 3 and 2 (0.72 and 0.37 of their bound), and its fp32 rounding reference does NOT show the excess (e32r 9.8e-6), so
the 4 * e32r leg does not carry it: the divisor does.

Structural checks in every case (bglu_cases.read_planes / read_skip / read_out / inputs_unchanged): outputs sit in
allocations filled with a NaN pattern (0x7fc0 in every uint16 of a plane tensor, float NaN elsewhere) with guards of the same
pattern in front of item 0 and behind item B; afterwards every own element is finite with no pattern left, guards and margins
(the frame above frame 0 unless nx_row0, HP_F0 bins either side, through hp_par_pos under nx_par) hold the pattern bit for bit,
the nx_row0 pad frame is hp_split of the broadcast conv1 bias bit for bit, dec writes every bin 0 .. Fo - 1 over its two phases
and nothing at bin 2 Fout1 + 1, dec1 leaves the other decoder's channel alone, inputs and weights are bit-identical; item B
(the dump target of lanes without a position) is unconstrained.

The element rule's ratios come close to 1 by construction (round-to-nearest of a value just above a power of two IS 2^-8 of it);
only the allowance is slack there.

Deliberately not here: values beyond the f16x2 window (tests/test_gpu_f16x2.py), the BGLU_DIAG builds, timing."""
import os
import re

import pytest
import torch

from conftest import pkg
from helpers import bglu_cases as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = []


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    lib = pkg("_lib")
    lib.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    yield lib
    path = os.environ.get("PDSE_BGLU_MARGINS")           # the table behind profiles/bglu_ops_margins.txt
    if path:
        with open(path, "w") as f:
            f.write("%-36s %-10s %-11s %-11s %-7s %s\n" % ("case", "tensor", "error", "bound", "ratio", "rule"))
            for case, name, err, bound, ratio, what in ROWS:
                f.write("%-36s %-10s %.3e   %.3e   %.3f   %s\n" % (case, name, err, bound, ratio, what))


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault fails every later launch of the process: stop instead of piling them on
        pytest.exit("device error after a block-kernel launch: %s" % e, returncode=3)


def _run(L, case):
    b = G.build(case, DEV)
    L.launch(b.desc)
    _sync()
    G.verify(b, ROWS)


@pytest.mark.parametrize("case", G.CASES[3], ids=G.by_id(G.CASES[3]))
def test_bglu_bf16x3(L, case):
    _run(L, case)


@pytest.mark.parametrize("case", G.CASES[2], ids=G.by_id(G.CASES[2]))
def test_bglu_f16x2(L, case):
    _run(L, case)


@pytest.mark.parametrize("case", G.CASES[1], ids=G.by_id(G.CASES[1]))
def test_bglu_bf16(L, case):
    _run(L, case)


@pytest.mark.parametrize("npl", [3, 2, 1])
def test_planes_conv(L, npl):
    """Decoder stage 5's conv1 of one or two weight sets over (cin0, cin1) in {(32, 0), (64, 0), (64, 32), (64, 64)} - every exit
    of the two-chunk K loop - T in {1, 9, 33}, B in {1, 3}, with and without bias: hp_join of every output against float64 by
    the fp32 rule (np = 1: within one bf16 rounding of it, element by element), NaN-pattern margins and dump item intact."""
    for case in [c for c in G.PC_CASES if c["np"] == npl]:
        b = G.build_pc(case, DEV)
        L.launch(b.desc)
        _sync()
        G.verify_pc(b, ROWS)


# ------------------------------------------------------------------ refusals
def _null(*names):
    return lambda d, b: [setattr(d, n, None) for n in names]


def _set(**kw):
    return lambda d, b: [setattr(d, k, v) for k, v in kw.items()]


def _elem(name, i, v):
    return lambda d, b: getattr(d, name).__setitem__(i, v)


def _bump(name, by, i=None):
    def f(d, b):
        if i is None:
            setattr(d, name, getattr(d, name) + by)
        else:
            getattr(d, name)[i] = getattr(d, name)[i] + by
    return f


ENC, ENC1, ENC5, DEC, DEC1 = ("encnp3_small_B3_T1_F19", "enc1np3_small_B3_T1_F25", "enc5np3_small_B3_T1_F9", "decnp3_small_B3_T1_F4",
                              "dec1np3_small_B3_T1_F9")
NULL, GEOM, MISSING = "bglu: null operand", r"bglu: bad geometry \(np in \{1, 2, 3\}", "bglu: an operand of the selected form is missing"
FIT, SLOPE = "bglu: the chained tile does not fit its hp tensor", "bglu: PReLU slope must be <= 1"
REFUSALS = [
    # (name, base case, mutation, message in csrc/bglu.hip)
    ("null_w0", ENC, _null("w0"), NULL), ("null_wlc", ENC, _null("wlc"), NULL), ("null_bc2", ENC, _null("bc2"), NULL),
    ("slope_1.5", ENC, _set(slope=1.5), SLOPE), ("slope_nan", ENC, _set(slope=float("nan")), SLOPE),
    ("np4", ENC, _set(np=4), GEOM), ("C2_32", ENC, _set(C2=32), GEOM), ("nx_n4", ENC, _set(nx_n=4), GEOM), ("ntaps11", ENC, _set(ntaps=11), GEOM),
    ("B0", ENC, _set(B=0), GEOM),
    ("Fout1_above_Fout", DEC, lambda d, b: setattr(d, "Fout1", d.Fout + 1), "bglu: Fout1 > Fout"),
    ("wc2_null_C2_64", ENC, _null("wc2"), MISSING), ("out_null_enc5", ENC5, _null("out"), MISSING), ("nx_hp_null", ENC, _null("nx_hp"), MISSING),
    ("nx_out0_null", ENC, _elem("nx_out", 0, None), MISSING), ("w2_null_p1mask", DEC, _null("w2"), MISSING),
    ("hp_null", ENC, _null("hp"), "bglu: null hp"),
    ("hp_par_sf_in_1", DEC, _set(hp_par=1), r"bglu: parity-split input planes \(hp_par = 1\) are for stride-2 taps"),
    ("hp_par_2", ENC, _set(hp_par=2), r"bglu: parity-split input planes \(hp_par = 1\) are for stride-2 taps"),
    ("hp_Tp_T", ENC, lambda d, b: setattr(d, "hp_Tp", d.Tout), "bglu: a tap leaves the margins of hp"),
    ("tap_df_one_beyond", ENC, lambda d, b: d.tap_df.__setitem__(5, d.hp_Fp - d.hp_f0 - 2 * (d.Fout - 1)), "bglu: a tap leaves the margins of hp"),
    ("enc1_x1_null", ENC1, lambda d, b: setattr(d.x1, "ptr", None), "bglu: encoder stage 1 needs two fp32 sources and the ten"),
    ("enc1_ntaps6", ENC1, _set(ntaps=6), "bglu: encoder stage 1 needs two fp32 sources and the ten"),
    ("nx_items_B", ENC, lambda d, b: setattr(d, "nx_items", d.B), r"bglu: nx_hp / nx_out need B \+ 1 allocated items"),
    ("nx_Fp_one_short", ENC, lambda d, b: setattr(d, "nx_Fp", d.Fout - 1 + d.nx_f0), FIT),      # one short of holding the last bin
    ("p1mask_without_nx_add", DEC, _null("nx_add"), FIT),
    ("nx_row0_nx_t0_0", ENC, _set(nx_row0=1, nx_t0=0), FIT),
    ("add_stride_not_4", DEC, _bump("add_st", 2), "bglu: the addend is kept in groups of four channels"),
    ("add_base_off_4_bytes", DEC, _bump("nx_add", 4), "bglu: the addend is kept in groups of four channels"),
    ("skip_stride_not_4", ENC, _bump("nx_st", 2, 1), "bglu: skip tensors are kept in groups of four channels"),
    ("qexp_41", ENC.replace("np3", "np2"), _elem("qexp", 1, 41), r"bglu: qexp \(f16x2 weight exponents\) out of range"),
    ("qexp_-41", ENC.replace("np3", "np2"), _elem("qexp", 3, -41), r"bglu: qexp \(f16x2 weight exponents\) out of range"),
    ("no_instantiation_ntaps5", ENC, _set(ntaps=5), "bglu: no instantiation for this"),
]
PC = "pc_np3_nd2_c64_64_T9_B3_bias"
PC_FORM, PC_F4 = "planes: the convolution form takes 1 or 2 weight sets", r"planes: the convolution form is built for F == 4"
PC_REFUSALS = [
    ("F5", PC, _set(F=5, hp_Fp=9), PC_F4), ("cin0_48", PC, _set(cin0=48), PC_FORM),
    ("cin_160", PC, _set(cin0=96), PC_FORM),             # 96 is a legal multiple of 32: the sum 96 + 64 = 160 > 128 is what is refused
    ("nd3", PC, _set(nd=3), PC_FORM),
    ("bias_misaligned", PC, _bump("bias", 4, 1), PC_F4),  # F stays 4 here; the source has one message for F and for the alignment
    ("nd2_without_hp1", PC, _null("hp1"), PC_FORM),
]
# every refusal the table is meant to hold, by name: an entry that slid into a comment cannot go unnoticed
assert len(REFUSALS) == 33 and len({r[0] for r in REFUSALS}) == 33 and "p1mask_without_nx_add" in {r[0] for r in REFUSALS} and len(PC_REFUSALS) == 6


def _refused(L, desc, name, message):
    said = None
    try:
        L.launch(desc)
    except L.PdseError as e:
        said = str(e)
    _sync()
    assert said is not None, "%s: not refused" % name
    assert re.search(message, said), (name, said)


def test_refusals(L):
    """Each descriptor must raise PdseError with the message in the source and launch nothing: the NaN-filled outputs stay as
    they were."""
    for name, cid, mutate, message in REFUSALS:
        b = G.build(G.find(cid), DEV)
        mutate(b.desc, b)
        _refused(L, b.desc, "bglu " + name, message)
        assert G.outputs_untouched(b), "bglu %s: a refused descriptor launched" % name
    for name, cid, mutate, message in PC_REFUSALS:
        b = G.build_pc(next(c for c in G.PC_CASES if c["id"] == cid), DEV)
        mutate(b.desc, b)
        _refused(L, b.desc, "planes " + name, message)
        assert all(bool((buf.cpu().numpy().view("uint16") == G.NAN16).all()) for buf in b.hpbuf), "planes %s: a refused descriptor launched" % name


def test_refusal_messages_are_the_sources():
    """The regexes above are taken from csrc/bglu.hip: each one finds a pdse_set_error there."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(pkg().__file__)), "csrc", "bglu.hip")).read()
    said = re.findall(r'pdse_set_error\("([^"]*)"\)', src)
    for _, _, _, message in REFUSALS + PC_REFUSALS:
        assert any(re.search(message, s) for s in said), message
