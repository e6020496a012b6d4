"""Host side of the spectral compression modes (``feat_type``: sqrt, normal, cubic, log_1x, none; no device needed): the float64
restatement of tests/helpers/feat_refs.py against the fixture made from the reference's own statements
(tests/golden/feat_type.npz, tools/make_golden_feattype.py), the trainer's validation of the value, the recorded descriptors and
the cache keys."""
import argparse
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, pkg

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import feat_refs as R  # noqa: E402

MODES = R.FEAT_TYPES


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return pkg("_lib")


def test_helper_agrees_with_the_reference_statements():
    """The fixture holds what the reference's fp32 tensor statements give; the helper is float64.  An fp32 chain of norm, one
    transcendental, atan2, cos / sin and a product is a handful of roundings of 2^-24 each: 4e-7 rel-L2 is more than 5 of them,
    and the measured distances (profiles/feat_type_parity.txt) are 6e-8 .. 2.7e-7.  The copies are exact.  The stored
    measurements are what this machine's numpy computes again."""
    g = golden("feat_type")
    x = g["input"]
    assert x.shape == (2, 2, 9, 161) and x.dtype == np.float32
    for t, f, re, im in g["planted"]:
        assert x[0, 0, int(t), int(f)] == np.float32(re) and x[0, 1, int(t), int(f)] == np.float32(im)
    for mode in MODES:
        for kind, want in (("comp", R.compress(x, mode)), ("dec", R.decompress(x, mode)), ("wav", R.wav_of(x, mode))):
            got = g["%s_%s" % (kind, mode)]
            assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(want).all()
            rel, mx = R.errors(got, want)
            long_name = {"comp": "compress", "dec": "decompress", "wav": "wav"}[kind]
            stored = g["err_%s_%s" % (long_name, mode)]
            print(mode, kind, rel, mx, stored)
            assert rel < 4e-7, (mode, kind)
            assert abs(rel - stored[0]) <= 1e-3 * stored[0] + 1e-12 and abs(mx - stored[1]) <= 1e-3 * stored[1] + 1e-30
    for kind, mode in (("comp", "none"), ("dec", "none"), ("dec", "normal")):
        assert np.array_equal(g["%s_%s" % (kind, mode)], x)
    # zero bins stay (f(0), 0) = (0, 0) in every transform, and the pairs are inverses of each other
    for mode in MODES:
        assert np.all(R.compress(x, mode)[0, :, 0, 0] == 0) and np.all(R.decompress(x, mode)[0, :, 0, 0] == 0)
        small = x[1]                                            # no planted bin: moderate magnitudes
        back = R.decompress(R.compress(small[None], mode), mode)
        assert np.abs(back - small).max() < 1e-12


def _config(feat_type):
    ns = argparse.Namespace
    return (ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav="y"),
            ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type=feat_type)))


@pytest.mark.parametrize("feat_type", MODES)
def test_trainer_accepts_the_five_values(lib, feat_type):
    """On a CPU context the constructor goes past its configuration checks and stops where it asks for the device."""
    args, config = _config(feat_type)
    with pytest.raises(lib.PdseError, match="needs an MI355X"):
        pkg("trainer").ComplexDDPMTrainer(args, config, device="cpu", prior_state_dict={}, ddpm_state_dict={})


@pytest.mark.parametrize("feat_type", ("foo", "SQRT", "", None))
def test_trainer_rejects_other_values(lib, feat_type):
    args, config = _config(feat_type)
    with pytest.raises(ValueError, match="'sqrt', 'normal', 'cubic', 'log_1x', 'none'"):
        pkg("trainer").ComplexDDPMTrainer(args, config, device="cpu", prior_state_dict={}, ddpm_state_dict={})
    with pytest.raises(ValueError, match="feat_type"):
        pkg("pipeline").SamplerPipeline("cpu", "GCRN", {}, {}, 1, L_=1600, feat_type=feat_type)
    import torch

    for fn in (pkg("ops").compress, pkg("ops").decompress, pkg("ops").spec_to_wav):
        with pytest.raises(ValueError, match="feat_type"):
            fn(torch.zeros(1, 2, 3, 161), feat_type)


def test_geometry_check_stays(lib):
    args, config = _config("cubic")
    config.train.win_shift = 128
    with pytest.raises(NotImplementedError, match="320/320/160"):
        pkg("trainer").ComplexDDPMTrainer(args, config, device="cpu", prior_state_dict={}, ddpm_state_dict={})


def _scalars(descs):
    import ctypes as C

    def scal(v):
        if isinstance(v, C.Structure):
            return {n: scal(getattr(v, n)) for n, t in v._fields_ if t is not C.c_void_p}
        if isinstance(v, C.Array):
            return None if v._type_ is C.c_void_p else [scal(e) for e in v]
        return v

    return [(type(d).__name__, tag, scal(d)) for d, tag in descs]


def _compands(lib, descs):
    return [d for d, _ in descs if isinstance(d, lib.CompandDesc)]


def test_sqrt_pipelines_record_what_they_recorded(lib, weights):
    """With and without the argument: the same descriptor types, tags and scalar fields, launch for launch; compand modes 0, 1."""
    P = pkg("pipeline").SamplerPipeline
    for kw in (dict(), dict(split="bf16x3"), dict(fast_sampling=False), dict(ragged=True), dict(objective=True), dict(label=True)):
        a = P("cpu", "GCRN", weights("GCRN"), weights("DiffUNet1"), 2, L_=1600, **kw)
        b = P("cpu", "GCRN", weights("GCRN"), weights("DiffUNet1"), 2, L_=1600, feat_type="sqrt", **kw)
        assert _scalars(a.descs) == _scalars(b.descs) and a.ranges == b.ranges, kw
        assert a.stft.ns == b.stft.ns == ("StftPlan", False, "stft", bool(a.split_bf16))
        want = [0] if kw.get("objective") else [0, 1]
        assert [d.mode for d in _compands(lib, a.descs)] == want, kw


def test_modes_record_their_descriptors(lib, weights):
    """The modes differ from the sqrt plan in the compand launches alone: their mode field, and "none" has no front-end launch."""
    P = pkg("pipeline").SamplerPipeline
    base = P("cpu", "GCRN", weights("GCRN"), weights("DiffUNet1"), 2, L_=1600)
    plain = [s for s in _scalars(base.descs) if s[0] != "CompandDesc"]
    want = {"normal": [lib.COMPAND_MAG, lib.COMPAND_COPY], "cubic": [lib.COMPAND_POW03, lib.COMPAND_POW103],
            "log_1x": [lib.COMPAND_LOG1X, lib.COMPAND_EXPM1], "none": [lib.COMPAND_COPY]}
    assert [lib.COMPAND_SQRT, lib.COMPAND_SQUARE, lib.COMPAND_MAG, lib.COMPAND_COPY, lib.COMPAND_POW03, lib.COMPAND_POW103,
            lib.COMPAND_LOG1X, lib.COMPAND_EXPM1] == list(range(8))
    for mode, modes in want.items():
        p = P("cpu", "GCRN", weights("GCRN"), weights("DiffUNet1"), 2, L_=1600, feat_type=mode)
        assert [d.mode for d in _compands(lib, p.descs)] == modes, mode
        assert [s for s in _scalars(p.descs) if s[0] != "CompandDesc"] == plain, mode
        back = _compands(lib, p.descs)[-1]
        assert back.F == 161 and back.out_st == 336 and back.out_sc == 168           # the ISTFT GEMM's frame-major rows, copy included
        b0, e0 = p.ranges["stft"]
        assert len(_compands(lib, p.descs[b0:e0])) == (0 if mode == "none" else 1)
    # the label leg's front on its own (a pipeline builds it on the device only)
    nets = pkg("nets")
    for mode in MODES:
        st = nets.StftPlan(nets.Ctx("cpu"), 2, 1600, feat_type=mode)
        st.build(prep=False)
        assert [d.mode for d in _compands(lib, st.descs)] == ([] if mode == "none" else [lib.COMPRESS_MODE[mode]])


def test_two_modes_share_no_cache_key(lib):
    nets, ops, T = pkg("nets"), pkg("ops"), pkg("trainer").ComplexDDPMTrainer
    ctx = nets.Ctx("cpu")
    assert len({nets.StftPlan(ctx, 1, 1600, feat_type=m).ns for m in MODES}) == 5
    assert len({nets.IstftPlan(ctx, 1, 11, 1600, feat_type=m).ns for m in MODES}) == 5
    assert len({ops._label_key("cuda:0", 2, 1600, False, m) for m in MODES}) == 5
    assert ops._label_key("cuda:0", 2, 1600, False, "sqrt") == ("cuda:0", 2, 1600, False, "sqrt")
    keys = set()
    for m in MODES:
        t = T.__new__(T)
        t.args, t.params, t.feat_type = argparse.Namespace(sigma=False), argparse.Namespace(fast_sampling=True), m
        keys.add(t._key(2, L_=1600, label=True))
        if m == "sqrt":
            assert t._key(2, L_=1600, ragged=True) == (2, None, 1600, False, True, True)     # the key it always had
    assert len(keys) == 5


def test_compand_rejects_unknown_modes_without_a_device(lib):
    import ctypes as C

    buf = (C.c_float * 8)()
    for mode in (-1, 8, 99):
        d = lib.CompandDesc()
        d.in_, d.out, d.plane, d.B, d.mode = C.addressof(buf), C.addressof(buf), 4, 1, mode
        with pytest.raises(lib.PdseError, match=r"compand: mode must be 0 \(mag\*\*0\.5\), 1 .* 7 \(exp\(mag\)-1\)"):
            lib.launch(d)
    good = dict(spec=8, basis=8, frames=8, B=1, T=4, F=161)
    for mode in (0, 2, 4, 6, 8, -1):
        with pytest.raises(lib.PdseError, match="spec_frames: mode must be a decompress mode"):
            lib.spec_frames_mode(mode=mode, **good)
    with pytest.raises(lib.PdseError, match="spec_frames: null"):
        lib.spec_frames_mode(**dict(good, spec=0, mode=5))
    with pytest.raises(lib.PdseError, match="F must be 161"):
        lib.spec_frames_mode(**dict(good, F=129, mode=3))
