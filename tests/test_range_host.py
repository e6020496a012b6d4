"""Host side of the range audit of the f16x2 window (csrc/range.hip, include/pdse.h: pdse_range_desc; no device needed): the
exported bin map, the descriptor layout against the header, the report's arithmetic and the argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg


def test_bin_table_matches_frexp_on_every_fp16_value():
    """RANGE_BINADE (the map csrc/range.hip documents in its header) against numpy.frexp on ALL 65536 fp16 bit patterns: every
    exponent, both signs, subnormals, zeros, infinities, NaN.  The host counterpart ``rangeaudit.histogram`` reads the table and
    must put every value where the definition says."""
    L, RA = pkg("_lib"), pkg("rangeaudit")
    assert len(L.RANGE_BINADE) == L.RANGE_BINS == 32
    assert L.RANGE_BINADE[0] is None and L.RANGE_BINADE[1] == float("-inf")
    assert list(L.RANGE_BINADE[2:31]) == list(range(-14, 15)) and L.RANGE_BINADE[31] == 15     # one bin per normal binade, top one apart
    assert L.RANGE_BINADE[L.RANGE_BIN_FULL] == -2 and L.RANGE_BIN_TOP == 31
    v = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float64)
    want = np.zeros(32, np.int64)
    for x in v:
        if not np.isfinite(x):
            b = 31
        elif x == 0:
            b = 0
        else:
            e = np.frexp(abs(x))[1] - 1                  # |x| in [2^e, 2^(e+1))
            b = 1 if e < -14 else (31 if e >= 15 else e + 16)
        want[b] += 1
    got = RA.histogram(v)
    assert got.tolist() == want.tolist()
    assert want[0] == 2 and want[1] == 2 * 1023 and want[31] == 2 * 1024 + 2 * 1024 and all(want[2:31] == 2 * 1024)
    # the exponent argument shifts the binade and nothing else
    assert RA.histogram([1.0, -1.5, 2.0 ** -19, 0.0, 2.0 ** 11], exp=4).tolist() == RA.histogram([16.0, -24.0, 2.0 ** -15, 0.0, 2.0 ** 15]).tolist()


def _c_struct(name):
    """[(type, field, array length)] of a struct of include/pdse.h."""
    src = open(os.path.join(ROOT, "include", "pdse.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = re.match(r"((?:const )?[\w ]+?[\s\*]+)(.*)", decl).groups()
        for n in names.split(","):
            out.append(("ptr" if "*" in typ else typ.replace("const", "").strip(), n.strip()))
    return out


def test_range_descriptor_layout_matches_the_header():
    L = pkg("_lib")
    size = {"ptr": 8, "int64_t": 8, "int32_t": 4, "uint32_t": 4}
    for cname, typ in (("pdse_range_row", L.RangeRow), ("pdse_range_desc", L.RangeDesc)):
        off = 0
        fields = _c_struct(cname)
        assert [n for _, n in fields] == [n for n, _ in typ._fields_]
        for ctype, n in fields:
            s = size[ctype]
            off = (off + s - 1) // s * s                 # natural alignment
            assert getattr(typ, n).offset == off and getattr(typ, n).size == s, (cname, n)
            off += s
        assert C.sizeof(typ) == (off + 7) // 8 * 8
    assert C.sizeof(L.RangeRow) == 80 and C.sizeof(L.RangeDesc) == 32
    hdr = open(os.path.join(ROOT, "include", "pdse.h")).read()
    assert re.search(r"PDSE_OP_RANGE = (\d+)", hdr).group(1) == str(L.OP_RANGE) == "31"
    assert re.search(r"#define PDSE_ABI_VERSION (\d+)", hdr).group(1) == str(L.ABI_VERSION) == "9"      # additive
    assert L.DESC_TYPES[L.OP_RANGE] is L.RangeDesc and "pdse_range_hist" in L.EXPORTS
    for macro, val in (("PDSE_RANGE_BINS", L.RANGE_BINS), ("PDSE_RANGE_F32", L.RANGE_F32), ("PDSE_RANGE_F16HI", L.RANGE_F16HI)):
        assert re.search(r"#define %s (\d+)" % macro, hdr).group(1) == str(val)


def _hist(**bins):
    h = [0] * 32
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


def test_report_arithmetic_on_hand_made_histograms():
    RA = pkg("rangeaudit")
    Row = RA.ReportRow
    mid = Row("mid", "step0", _hist(b0=5, b14=10, b18=30, b10=10))            # bins 14 and 18 are inside, bin 10 under the edge
    assert mid.count == 55 and mid.nonzero == 50 and mid.max_binade == 2 and mid.below_frac == pytest.approx(0.2)
    assert not mid.below and not mid.above and mid.ok
    edge = Row("edge", "step0", _hist(b13=7, b1=1))                            # largest binade 2^-3: just under the edge
    assert edge.below and not edge.above and edge.max_binade == -3 and edge.below_frac == 1.0 and not edge.ok
    just = Row("just", "step0", _hist(b14=1, b2=99))                           # one element at 2^-2: not below, 99 % under
    assert not just.below and just.below_frac == pytest.approx(0.99) and just.max_binade == -2
    sub = Row("sub", "prior", _hist(b1=4))
    assert sub.below and sub.max_binade == float("-inf")
    top = Row("top", "step1", _hist(b31=1, b20=100))
    assert top.above and not top.below and top.max_binade == 15 and not top.ok
    both = Row("both", "step1", _hist(b31=2, b3=5))                            # bin 31 is the highest occupied bin: above, not below
    assert both.above and not both.below
    zero = Row("zero", "prior", _hist(b0=64))                                  # all zero: neither, and no division by zero
    assert zero.count == 64 and zero.max_binade is None and zero.below_frac == 0.0 and not zero.below and not zero.above and zero.ok
    with pytest.raises(ValueError):
        Row("short", "prior", [0] * 31)

    rep = RA.RangeReport([mid, just, zero])
    assert rep.ok and rep.worst() is just and len(rep) == 3 and rep.below() == [] and rep.above() == []
    rep = RA.RangeReport([mid, edge, sub, zero])
    assert not rep.ok and rep.worst() is edge and rep.below() == [edge, sub]
    rep = RA.RangeReport([edge, top, both])
    assert not rep.ok and rep.worst() is top and rep.above() == [top, both]
    assert RA.RangeReport([]).ok and RA.RangeReport([]).worst() is None
    text = str(RA.RangeReport([mid, edge, top, zero]))
    assert text.count("\n") == 4 and "BELOW" in text and "ABOVE" in text and "edge" in text


def test_layout_boxes_agree_with_the_join_helpers():
    """packing.hp_box / tcm2_hs_box name exactly the elements hp_join / tcm2_join_h return: a walk over the box, done here with
    numpy as csrc/range.hip does it, collects the hi plane of the same logical tensor (any parity), margins and lo excluded."""
    P = pkg("packing")
    rng = np.random.default_rng(3)
    B, T, F = 2, 5, 9
    x = rng.standard_normal((B, 32, T, F)).astype(np.float32)
    hp = P.hp_split(x, 2)

    def walk(buf, box):
        flat, out = buf.reshape(-1), []
        n0, n1, n2, n3 = box["dims"]
        s0, s1, s2 = box["strides"]
        for i0 in range(n0):
            for i1 in range(n1):
                for i2 in range(n2):
                    for i3 in range(n3):
                        i = i3 + box["i0"]
                        pos = (i & 1) * box["par_half"] + (i >> 1) if box["par_half"] else i
                        a = box["off"] + i0 * s0 + i1 * s1 + i2 * s2 + 8 * pos
                        out.append(flat[a:a + 8])
        return np.concatenate(out)

    for par in (False, True):
        buf = hp.copy()
        if par:                                                               # store the bins split by parity, margins included
            Fp = buf.shape[4]
            tmp = np.zeros_like(buf)
            tmp[:, :, :, :, P.hp_par_pos(Fp)] = buf
            buf = tmp
        buf[:, 0] = 0x3c00                                                    # a pad frame that is not zero must not be counted
        got = walk(buf, P.hp_box(B, T, F, 2, par=par))
        # element for element, in the walk's order (b, t, g, f, e): plane 0 of the natural-order tensor over hp_join's index set
        assert np.array_equal(got, hp[:, P.HP_T0:, :, 0, P.HP_F0:P.HP_F0 + F, :].reshape(-1))
        assert got.size == P.hp_join(buf, par=par).size == x.size
        assert np.array_equal(P.hp_join(buf, par=par), P.hp_join(hp))         # the parity-aware join returns the same logical tensor
    vm, vk = rng.standard_normal((2, B, 64, T)).astype(np.float32)
    hs = P.tcm2_split_h(vm, vk, 2)
    for br, v in enumerate((vm, vk)):
        got = walk(hs, P.tcm2_hs_box(B, T, 2, br))
        assert np.array_equal(got, hs[:, br, :, :, 0, P.TCM2_HS_PAD:P.TCM2_HS_PAD + T, :].reshape(-1))     # order (b, kb kg, t, e)
        assert got.size == v.size


def test_make_row_refuses_what_does_not_fit():
    import torch

    L, RA, P = pkg("_lib"), pkg("rangeaudit"), pkg("packing")
    t = torch.zeros(P.hp_shape(3, 5, 9, 2), dtype=torch.int16)
    row = RA.make_row(t, L.RANGE_F16HI, 0, P.hp_box(2, 5, 9, 2, par=True), 7)
    assert row.n == 2 * 32 * 5 * 9 and row.out_row == 7 and row.par_half == 7 and row.i0 == 2
    with pytest.raises(ValueError):
        RA.make_row(t, L.RANGE_F16HI, 0, P.hp_box(4, 5, 9, 2), 0)             # more items than the tensor holds
    with pytest.raises(ValueError):
        RA.make_row(t, 5, 0, None, 0)
    with pytest.raises(ValueError):
        RA.make_row(torch.zeros(4, 4).t(), L.RANGE_F32, 4, None, 0)           # not contiguous
    f = RA.make_row(torch.zeros(3, 5), L.RANGE_F32, 4, None, 1)
    assert f.n == 15 and f.exp == 4
    assert RA.work_blocks([f]) == 1 and RA.work_blocks([row, f]) == 1


def test_audit_arguments(weights):
    """audit=True with split="bf16x3" is accepted and records nothing; range_report() on a pipeline built without the audit
    raises ValueError; the audited() contract of a builder lists the plane tensors of an f16x2 plan and nothing on bf16x3."""
    L = pkg("_lib")
    P = pkg("pipeline").SamplerPipeline
    plain = P("cpu", "GCRN", weights("GCRN"), weights("DiffUNet1"), 1, L_=1600)
    with pytest.raises(ValueError, match="audit"):
        plain.range_report()
    b3 = P("cpu", "GCRN", weights("GCRN"), weights("DiffUNet1"), 1, L_=1600, split="bf16x3", audit=True)
    assert b3.audit and not b3.audited and len(b3.descs) == len(plain.descs)
    assert not any(isinstance(d, L.RangeDesc) for d, _ in b3.descs)
    rep = b3.range_report()
    assert len(rep) == 0 and rep.ok
    assert b3.eps.audited() == [] and b3.prior.audited() == []
    names = [n for n, *_ in plain.eps.audited()]
    assert {"hp_en2", "hp_en5", "hp_de1", "hp_de5", "hp_de5b", "tcm_hs0.main", "tcm_hs1.mask", "x", "x_init"} <= set(names)
    assert len(names) == len(set(names))
    assert all(n.startswith("gcrn.") for n, *_ in plain.prior.audited()) and len(plain.prior.audited()) >= 8
    with pytest.raises(ValueError):
        pkg("trainer").ComplexDDPMTrainer.__init__(object.__new__(pkg("trainer").ComplexDDPMTrainer), None, None, split="fp8")
