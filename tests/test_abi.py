"""CPU: the C-ABI library loads here (no GPU) and exports every symbol include/pdse.h
declares; descriptor layouts of the ctypes binding match the compiled structs; argument
errors are reported through the status/last_error convention without touching a device."""
import os
import re

import pytest

from conftest import ROOT, pkg


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return pkg("_lib")


def test_header_symbols_all_exported(lib):
    text = open(os.path.join(ROOT, "include", "pdse.h")).read()
    declared = set(re.findall(r"\b(pdse_[a-z0-9_]+)\s*\(", text))
    declared -= {"pdse_plan"}
    assert len(declared) >= 20
    handle = lib.load()
    for name in sorted(declared):
        assert hasattr(handle, name), name
    assert set(lib.EXPORTS) == declared


def test_descriptor_sizes_match(lib):
    import ctypes as C

    handle = lib.load()
    for kind, typ in lib.DESC_TYPES.items():
        assert handle.pdse_desc_size(kind) == C.sizeof(typ), typ.__name__
    assert handle.pdse_desc_size(99) == -1


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdse.h")).read(), flags=re.S)


def _mirror_key(name):
    """pdse_xyz_desc and XyzDesc name the same struct: case and underscores do not count."""
    name = name.lower().replace("_", "")
    return name[4:] if name.startswith("pdse") else name


def _mirrors(lib):
    import ctypes as C

    found = [v for v in vars(lib).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure]
    table = {_mirror_key(v.__name__): v for v in found}
    assert len(table) == len(found)
    return table


def _header_structs():
    """Every struct typedef of include/pdse.h as a ctypes structure built from its declaration (a test helper, not a binding)."""
    import ctypes as C

    text = _header_text()
    bounds = {k: int(v) for k, v in re.findall(r"^#define\s+(\w+)\s+(\d+)\s*$", text, flags=re.M)}
    types = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "unsigned long long": C.c_ulonglong}
    item = r"\w+(?:\[\w+\])?"
    structs = {}
    for name, body in re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", text, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"(?:const\s+)?([a-z]\w*(?: long long)?)\s*(\*?)\s*(%s(?:\s*,\s*%s)*)" % (item, item), decl)
            assert m, (name, decl)
            base, star, names = m.groups()
            names = re.split(r"\s*,\s*", names)
            assert not star or len(names) == 1, (name, decl)     # `T* a, b` would make only a a pointer
            typ = C.c_void_p if star else types[base]
            for n in names:
                n, _, dim = n.partition("[")
                dim = dim.rstrip("]")
                fields.append((n, typ * (int(dim) if dim.isdigit() else bounds[dim]) if dim else typ))
        types[name] = structs[name] = type(name, (C.Structure,), {"_fields_": fields})
    return structs


def test_operator_table_matches_header(lib):
    """include/pdse.h names each operator three times - PDSE_OP_<KIND>, pdse_<kind>_desc and the direct entry that takes that
    descriptor; a row of _lib.OPS must bind exactly those three together, with no row and no declaration left over."""
    text = _header_text()
    kinds = {k: int(n) for k, n in re.findall(r"\bPDSE_OP_(\w+)\s*=\s*(\d+)", text)}
    entries = dict(re.findall(r"^int (pdse_\w+)\(const (pdse_\w+_desc)\* d, pdse_stream_t s\);", text, flags=re.M))
    mirrors = _mirrors(lib)
    assert len(kinds) == len(set(kinds.values())) == len(entries) == len(lib.OPS) == 32
    rows = {}
    for kind, typ, entry in lib.OPS:
        assert kind not in rows, kind
        rows[kind] = (typ, entry)
    used = set()
    for name, n in kinds.items():
        assert getattr(lib, "OP_" + name) == n, name
        typ, entry = rows.pop(n)
        struct = "pdse_%s_desc" % name.lower()
        assert entries.get(entry) == struct, (name, entry)
        assert mirrors[_mirror_key(struct)] is typ, (name, typ.__name__)
        used.add(entry)
    assert not rows and used == set(entries)
    assert [k for k, _, _ in lib.OPS] == sorted(kinds.values())
    assert lib.DESC_TYPES == {k: t for k, t, _ in lib.OPS} and lib.KIND_OF == {t: k for k, t, _ in lib.OPS}
    assert lib._DIRECT == {k: e for k, _, e in lib.OPS} and used <= set(lib.EXPORTS)


def test_descriptor_layouts_match_header(lib):
    """Field by field, not just sizeof: the same fields in the same order, each with the header's name (a trailing underscore
    may be added: `in` is a Python keyword), offset and size, and a pointer exactly where the header has one."""
    import ctypes as C

    def is_pointer(t):
        while hasattr(t, "_length_"):
            t = t._type_
        return t is C.c_void_p

    structs, mirrors = _header_structs(), _mirrors(lib)
    assert {_mirror_key(n) for n in structs} == set(mirrors) and len(structs) == len(mirrors) == 34
    for name, want in structs.items():
        have = mirrors[_mirror_key(name)]
        assert len(have._fields_) == len(want._fields_) and C.sizeof(have) == C.sizeof(want), name
        for (hn, ht), (wn, wt) in zip(have._fields_, want._fields_):
            assert hn in (wn, wn + "_"), (name, hn, wn)
            h, w = getattr(have, hn), getattr(want, wn)
            assert (h.offset, h.size) == (w.offset, w.size), (name, hn)
            assert is_pointer(ht) == is_pointer(wt), (name, hn)


def test_argument_errors_do_not_need_a_device(lib):
    with pytest.raises(lib.PdseError, match="null"):
        lib.launch(lib.GconvDesc())
    d = lib.LstmDesc()
    with pytest.raises(lib.PdseError, match="lstm"):
        lib.launch(d)
    with pytest.raises(lib.PdseError, match="bglu: null"):
        lib.launch(lib.BgluDesc())
    with pytest.raises(lib.PdseError, match="planes"):
        lib.launch(lib.PlanesDesc())
    with pytest.raises(lib.PdseError, match="glstmp"):
        lib.launch(lib.GlstmpDesc())
    with pytest.raises(lib.PdseError, match="tcm2s"):
        lib.launch(lib.Tcm2sDesc())
    assert lib.load().pdse_bglu_set_form(7) == -2 and lib.load().pdse_bglu_set_form(0) in (-1, 0)      # the product library holds form 0 only
    # round 3 (ABI 5): channel-blocked sources are a feature of the korder-3 kernel; the split GRU is the fused H = 64 form
    import ctypes as C

    buf = (C.c_float * 64)()
    ptr = C.addressof(buf)
    g = lib.GconvDesc()
    g.in0 = lib.Src(ptr, 64, 8, 8, 8, 16, 0, 8, 0)
    g.out, g.w0, g.taps = ptr, ptr, ptr
    g.B, g.Tout, g.Fout, g.Cout, g.ntaps, g.out_cr, g.korder, g.ksteps = 1, 1, 1, 32, 1, 1, 1, 8
    with pytest.raises(lib.PdseError, match="channel-blocked"):
        lib.launch(g)
    r = lib.GruDesc()
    r.whh, r.bhh, r.y, r.gx = ptr, ptr, ptr, ptr
    r.B, r.T, r.F, r.H, r.axis, r.split = 1, 1, 1, 128, 1, 1
    with pytest.raises(lib.PdseError, match="split-bf16"):
        lib.launch(r)
    n = lib.LnDesc()
    n.in_, n.gamma, n.beta, n.out = ptr, ptr, ptr, ptr
    n.B, n.T, n.N, n.r, n.blk = 1, 1, 8, 4, 3
    with pytest.raises(lib.PdseError, match="blk"):
        lib.launch(n)
    p = lib.Plan()
    assert len(p) == 0
    p.add(lib.EwDesc())
    assert len(p) == 1
    with pytest.raises(lib.PdseError, match="ew"):
        p.run()            # validation fails before any launch


def test_product_refuses_cpu(lib):
    import argparse

    ns = argparse.Namespace
    args = ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav="y")
    config = ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt"))
    with pytest.raises(lib.PdseError):
        pkg("trainer").ComplexDDPMTrainer(args, config, device="cpu", prior_state_dict={}, ddpm_state_dict={})
    with pytest.raises(lib.PdseError):
        pkg("ops").DiffUNet1Op({}, "cpu")


def test_generated_block_schedule_is_current(tmp_path, monkeypatch):
    """csrc/bglu_sched.inc is generated (tools/gen_bglu_sched.py): the committed file must be what the generator writes, and
    every variant's schedule must place each mm of an accumulate chain in program order and each vector chunk behind its
    producers."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_bglu_sched", os.path.join(ROOT, "tools", "gen_bglu_sched.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    committed = open(gen.OUT).read()
    monkeypatch.setattr(gen, "OUT", str(tmp_path / "sched.inc"))
    gen.main()
    assert open(str(tmp_path / "sched.inc")).read() == committed
    for name, var in gen.VARIANTS:
        M, V = gen.build(var)
        slots = gen.schedule(M, V)
        at = {}
        for i, (pm, pv) in enumerate(slots):
            for it in (pm, pv):
                if it is not None:
                    at[it] = i
        assert set(at) == set(M) | set(V), name
        for it, i in at.items():
            for dep in it.deps:
                gap = i - at[dep]
                assert gap >= (2 if (it.kind, dep.kind) == ("V", "M") else 1 if it.kind != dep.kind else 0), (name, it.name, dep.name)
