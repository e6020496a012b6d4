"""Host side of the posterior ensembles (``members=K``; no device needed): the recorded plans, the refusals, the C entry point's
argument errors, the float64 yardstick of tests/helpers/ensemble_refs.py against a naive formulation, and the draw order."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ensemble_refs as E  # noqa: E402

from test_feat_type_host import _scalars  # noqa: E402  (the comparison of recorded descriptors: types, tags, scalar fields)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return pkg("_lib")


def _pipe(weights, ddpm="DiffUNet1", B=2, **kw):
    return pkg("pipeline").SamplerPipeline("cpu", "GCRN", weights("GCRN"), weights(ddpm), B, L_=1600, **kw)


CASES = (("plain", "DiffUNet1", dict()), ("use_sigma", "DiffUNet1", dict(use_sigma=True)), ("deltamu", "Nocon", dict(deltamu=True)),
         ("cond_feat", "DiffUNet1", dict(cond="feat")), ("label", "DiffUNet1", dict(label=True)))


@pytest.mark.parametrize("name,ddpm,kw", CASES, ids=[c[0] for c in CASES])
def test_one_member_records_todays_plan(lib, weights, name, ddpm, kw):
    a, b = _pipe(weights, ddpm, **kw), _pipe(weights, ddpm, members=1, **kw)
    assert _scalars(a.descs) == _scalars(b.descs) and a.ranges == b.ranges
    assert b.members == 1 and b.members_spec is b.spec and tuple(b.xT_in.shape) == (2, 2, 11, 161)


def _ew(lib, pipe, rng):
    b, e = pipe.ranges[rng]
    return [d for d, _ in pipe.descs[b:e] if isinstance(d, lib.EwDesc)]


@pytest.mark.parametrize("name,ddpm,kw", CASES, ids=[c[0] for c in CASES])
def test_three_members_front_at_B_loop_at_3B(lib, weights, name, ddpm, kw):
    B, K = 2, 3
    one, p = _pipe(weights, ddpm, **kw), _pipe(weights, ddpm, members=K, **kw)
    n = B * 2 * 11 * 161
    # the front and the prior: launch for launch the one-member plan's, at B
    for rng in ("stft", "prior"):
        (b0, e0), (b1, e1) = one.ranges[rng], p.ranges[rng]
        assert _scalars(one.descs[b0:e0]) == _scalars(p.descs[b1:e1]), rng
    assert p.prior.B == B and p.eps.B == K * B and tuple(p.eps.x.shape) == (K * B, 2, 11, 161)
    # the prologue: K broadcast divisions per broadcast tensor, n floats each, the outputs n * 4 bytes apart
    div = [d for d in _ew(lib, p, "prologue") if d.op == lib.EW_DIV]
    groups = 2 if kw.get("cond") == "feat" else 1
    assert len(div) == K * groups and len([d for d in _ew(lib, one, "prologue") if d.op == lib.EW_DIV]) == groups
    for g in range(groups):
        part = div[g * K:(g + 1) * K]
        assert all(d.n == n and d.a == part[0].a for d in part)
        assert [d.out - part[0].out for d in part] == [4 * n * k for k in range(K)]
    assert div[0].a == p.prior.out.data_ptr() and div[0].out == p.init.data_ptr()
    if groups == 2:
        assert div[K].a == p.feat.data_ptr() and div[K].out == p.eps.x_init.data_ptr()
    # every other element-wise launch works on the K B rows
    rest = [d for rng in p.ranges if rng == "prologue" or rng.startswith("step") for d in _ew(lib, p, rng) if d.op != lib.EW_DIV]
    assert rest and all(d.n == K * n for d in rest)
    sig = [d for d, _ in p.descs if isinstance(d, lib.SigmaDesc)]
    assert len(sig) == (1 if kw.get("use_sigma") else 0) and all(d.nplanes == 2 * K * B and d.plane == 11 * 161 for d in sig)
    # the ranges are those of the one-member plan, every step present
    assert list(p.ranges) == list(one.ranges) and all("step%d" % i in p.ranges for i in range(p.nsteps))
    assert p.xT_in.shape[0] == K * B and tuple(p.members_spec.shape) == (K * B, 2, 11, 161) and tuple(p.spec.shape) == (B, 2, 11, 161)
    assert tuple(p.init.shape) == (K * B, 2, 11, 161)
    last = _ew(lib, p, "step0")[-1]
    assert last.op == lib.EW_UPDATE_FINAL and last.out == p.members_spec.data_ptr() and p.members_spec.data_ptr() != p.spec.data_ptr()
    assert p.istft.spec.data_ptr() == p.spec.data_ptr()               # the back end inverts the mean
    assert tuple(p.eps.tsteps.shape) == (p.nsteps, K * B)


@pytest.mark.parametrize("feat_type", ("sqrt", "normal", "cubic", "log_1x", "none"))
def test_members_with_every_feat_type_and_arithmetic(lib, weights, feat_type):
    for kw in (dict(), dict(split="bf16x3"), dict(dtype="bf16"), dict(fast_sampling=False)):
        p = _pipe(weights, members=2, feat_type=feat_type, **kw)
        assert p.eps.B == 4 and p.feat_type == feat_type


def test_refusals_of_the_plan(lib, weights):
    P = pkg("pipeline").SamplerPipeline
    for bad in (0, 17, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="members must be an integer in 1 .. 16"):
            _pipe(weights, members=bad)
    for flag in ("ragged", "verdict", "objective"):
        with pytest.raises(ValueError, match="members=3 with %s=True" % flag):
            _pipe(weights, members=3, **{flag: True})
        _pipe(weights, members=1, **{flag: True})                     # one member: as ever
    p = _pipe(weights, members=3)
    with pytest.raises(ValueError, match="members=3.*planfile.save_pipeline"):
        pkg("planfile").save_pipeline("unused.pdse", p)
    x = torch.zeros(6, 2, 11, 161)
    with pytest.raises(ValueError, match="graph=True with members=3"):
        p.enhance(torch.zeros(2, 1600), x, graph=True)
    with pytest.raises(ValueError, match="graph=True with members=3"):
        p.sample(torch.zeros(2, 2, 11, 161), x, graph=True)
    with pytest.raises(ValueError, match="graph=True with members=3"):
        p.run(graph=True)
    with pytest.raises(ValueError, match="x_T: expected"):
        p.enhance(torch.zeros(2, 1600), torch.zeros(2, 2, 11, 161))
    with pytest.raises(lib.PdseError, match="CPU context"):           # both x_T layouts pass the geometry check
        p.enhance(torch.zeros(2, 1600), torch.zeros(3, 2, 2, 11, 161))
    assert P is not None


def _bare_trainer(device="cpu", **attrs):
    T = pkg("trainer").ComplexDDPMTrainer
    t = T.__new__(T)
    t.args, t.params, t.feat_type = argparse.Namespace(sigma=False, generated_wav="unused"), argparse.Namespace(fast_sampling=True), "sqrt"
    t.device, t.channels, t.audit = torch.device(device), "mix", False
    for k, v in attrs.items():
        setattr(t, k, v)
    return t


def test_refusals_of_the_trainer(lib):
    t = _bare_trainer()
    assert t._key(2, L_=1600) == (2, None, 1600, False, True) == t._key(2, L_=1600, members=1)
    assert t._key(2, L_=1600, members=3) == (2, None, 1600, False, True, ("members", 3))
    assert len({t._key(2, L_=1600, label=True, members=k) for k in (1, 2, 3)}) == 3
    wavs = [torch.zeros(400), torch.zeros(300)]
    for bad in (0, 17):
        for call in (lambda: t.enhance(torch.zeros(1, 400), members=bad), lambda: t.sample(torch.zeros(1, 2, 3, 161), members=bad),
                     lambda: t.enhance_batch(wavs, members=bad), lambda: t.enhance_members(torch.zeros(1, 400), members=bad),
                     lambda: t.validate_batch(wavs, wavs, members=bad), lambda: t.validate(members=bad),
                     lambda: t.generate_wav(members=bad)):
            with pytest.raises(ValueError, match="members must be an integer in 1 .. 16"):
                call()
    with pytest.raises(ValueError, match=r"enhance_batch\(exact=True, members=2\)"):
        t.enhance_batch(wavs, exact=True, members=2)
    with pytest.raises(ValueError, match=r"validate_batch\(exact=True, members=2\)"):
        t.validate_batch(wavs, wavs, exact=True, members=2)
    with pytest.raises(ValueError, match=r"validate\(exact=True, members=2\)"):
        t.validate(exact=True, members=2)
    with pytest.raises(ValueError, match=r"generate_wav\(members=2\) with batch > 1"):
        t.generate_wav(batch=2, members=2)
    with pytest.raises(ValueError, match=r"generate_wav\(members=2\) with inflight > 1"):
        t.generate_wav(inflight=2, members=2)
    with pytest.raises(ValueError, match=r"generate_wav\(members=2\) with channels='each'"):
        _bare_trainer(channels="each").generate_wav(members=2)
    with pytest.raises(ValueError, match=r"generate_wav\(members=2\) with audit=True"):
        _bare_trainer(audit=True).generate_wav(members=2)


@pytest.mark.parametrize("argv,msg", (
    (["--generate", "--members", "2", "--batch", "2"], "--members with --batch"),
    (["--generate", "--members", "2", "--inflight", "2"], "--members with --inflight"),
    (["--generate", "--members", "2", "--per-channel"], "--members with --per-channel"),
    (["--generate", "--members", "2", "--audit-range"], "--members with --audit-range"),
    (["--eval", "--objective", "--members", "2"], "--objective --members"),
    (["--generate", "--members", "0"], "--members must be 1 .. 16"),
    (["--generate", "--members", "17"], "--members must be 1 .. 16"),
))
def test_refusals_of_the_cli(lib, capsys, argv, msg):
    with pytest.raises(SystemExit) as e:
        pkg("main").parse_args_and_config(argv)
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_cli_flag_is_marked_and_defaults_to_one(lib, capsys):
    with pytest.raises(SystemExit):
        pkg("main").parse_args_and_config(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--members MEMBERS (not a flag of the reference)" in text and "default 1" in text


def test_entry_point_is_exported_and_the_abi_stays(lib):
    assert "pdse_ensemble_stats" in lib.EXPORTS and hasattr(lib.load(), "pdse_ensemble_stats")
    assert lib.ABI_VERSION == 9 == lib.load().pdse_abi_version()
    assert lib.ENSEMBLE_MAX == 16 and lib.ENSEMBLE_BLOCKS == 32
    text = open(os.path.join(ROOT, "include", "pdse.h")).read()
    assert "#define PDSE_ENSEMBLE_MAX 16\n" in text and "#define PDSE_ENSEMBLE_BLOCKS 32\n" in text


def test_argument_errors_do_not_need_a_device(lib):
    buf = (C.c_double * 64)()
    ptr = C.addressof(buf)
    frames = np.array([3, 2], dtype=np.int32)
    good = dict(members=ptr, mean=ptr, spread=ptr, frames_host=frames.ctypes.data, frames=ptr, partial=ptr, per_utt=ptr, per_member=ptr,
                K=2, B=2, T=3, F=161)
    for name in ("members", "mean", "spread", "frames_host", "frames", "partial", "per_utt", "per_member"):
        with pytest.raises(lib.PdseError, match="ensemble_stats: null pointer"):
            lib.ensemble_stats(**dict(good, **{name: 0}))
    for K in (0, 17, -1):
        with pytest.raises(lib.PdseError, match=r"ensemble_stats: K outside \[1, 16\]"):
            lib.ensemble_stats(**dict(good, K=K))
    for B in (0, 65536):
        with pytest.raises(lib.PdseError, match=r"ensemble_stats: B outside \[1, 65535\]"):
            lib.ensemble_stats(**dict(good, B=B))       # checked before frames_host is read
    for kw in (dict(T=0), dict(F=0)):
        with pytest.raises(lib.PdseError, match="ensemble_stats: bad sizes"):
            lib.ensemble_stats(**dict(good, **kw))
    for bad in ([4, 0], [0, -1]):
        fr = np.array(bad, dtype=np.int32)
        with pytest.raises(lib.PdseError, match=r"ensemble_stats: frames outside \[0, T\]"):
            lib.ensemble_stats(**dict(good, frames_host=fr.ctypes.data))
    ops = pkg("ops")
    with pytest.raises(ValueError, match="members must be an integer"):
        ops.ensemble_stats(torch.zeros(2, 2, 3, 161), 0, [3])
    with pytest.raises(lib.PdseError, match="GPU only"):
        ops.ensemble_stats(torch.zeros(2, 2, 3, 161), 2, [3])


@pytest.mark.parametrize("K,B,T,frames", ((2, 1, 1, (1,)), (3, 3, 5, (5, 1, 0)), (16, 2, 7, (7, 4)), (5, 1, 4, (4,))))
def test_reference_agrees_with_a_naive_formulation(K, B, T, frames):
    """The yardstick follows the definitions (members added in order, in double); numpy's own mean and variance of the
    complex128 members pair their additions differently.  The fp32 mean is the double mean rounded once, and two double
    means a few 2^-53 apart round to the same fp32 but for a tie: equal after rounding.  Everything else: 1e-12 relative."""
    rng = np.random.default_rng(7 * K + T)
    x = rng.standard_normal((K, B, 2, T, 161)).astype(np.float32)
    x[:, B - 1, :, 0] = x[0, B - 1, :, 0]                                   # one frame with all members equal
    got = E.ensemble_stats(x.reshape(K * B, 2, T, 161), K, frames)
    z = x[:, :, 0].astype(np.complex128) + 1j * x[:, :, 1].astype(np.complex128)     # [K,B,T,F]
    mean = np.mean(z, axis=0)
    assert np.array_equal(got["mean"][:, 0], mean.real.astype(np.float32)) and np.array_equal(got["mean"][:, 1], mean.imag.astype(np.float32))
    assert got["mean"].dtype == np.float32 and got["spread"].dtype == np.float32

    def close(a, b):
        return np.all(np.abs(a - b) <= 1e-12 * np.abs(b))

    var = np.var(z, axis=0, ddof=1) if K > 1 else np.zeros((B, T, 161))
    # the spread is rounded to fp32 once: half an fp32 ulp (2^-24 relative) beside the 1e-12 of the double behind it
    assert np.all(np.abs(got["spread"].astype(np.float64) - np.sqrt(var)) <= (2.0 ** -24 + 1e-12) * np.sqrt(var))
    assert np.all(got["spread"][B - 1, 0] == 0)
    for b in range(B):
        fr = frames[b]
        dev = np.abs(z[:, b, :fr] - mean[None, b, :fr]) ** 2
        assert close(got["per_utt"][b, 0], dev.sum()) and close(got["per_utt"][b, 1], (np.abs(mean[b, :fr]) ** 2).sum())
        assert close(got["per_member"][:, b], dev.reshape(K, -1).sum(axis=1))
        if K > 1 and fr:
            assert close(got["per_utt"][b, 0] / (K - 1), var[b, :fr].sum())
    if K > 1 and min(frames) > 0:
        assert close(E.relative_spread(got["per_utt"], K), np.sqrt([var[b, :frames[b]].sum() / (np.abs(mean[b, :frames[b]]) ** 2).sum()
                                                                    for b in range(B)]))


def test_draw_order_is_that_of_consecutive_passes(lib):
    t = _bare_trainer()
    shape = (2, 2, 5, 161)
    torch.manual_seed(11)
    three = t._x_T(shape, None, members=3)
    torch.manual_seed(11)
    ones = [t._x_T(shape, None) for _ in range(3)]
    assert tuple(three.shape) == (6, 2, 5, 161) and torch.equal(three, torch.cat(ones))
    torch.manual_seed(11)
    assert torch.equal(t._x_T(shape, None, members=1), ones[0]) and torch.equal(t._x_T(shape, None), ones[1])
    given = torch.arange(3 * 2 * 2 * 5 * 161, dtype=torch.float32).reshape(3, 2, 2, 5, 161)
    assert torch.equal(t._x_T(shape, given, members=3), given.reshape(6, 2, 5, 161))
    assert t._x_T(shape, given.reshape(6, 2, 5, 161), members=3).shape == (6, 2, 5, 161)
    assert torch.equal(t._x_T(shape, given[:1], members=1), given[0])              # [1,B,2,T,161]: one member
