"""CPU: the quality metrics' host side - the numpy restatement of the kernel arithmetic against the reference's fixtures
(this is where the GPU tolerances come from), frame counts and the rounding rule, the composite table, argument errors
without a device, and the command line's pairing."""
import os

import numpy as np
import pytest

import emu_metrics as E
from conftest import GOLDEN, pkg


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return pkg("_lib")


def test_emulation_matches_the_reference_fixtures():
    """The distances asserted here are the EMU_DISTANCE the GPU tolerances are ten times of.  PDSE_METRICS_PARITY=<file>
    writes the measured values (profiles/metrics_parity.txt)."""
    worst = dict.fromkeys(E.KEYS, 0.0)
    lines = []
    for name in E.CASES:
        g = E.load_case(name)
        r = E.emulate(*E.case_inputs(g))
        row = "%-16s" % name
        for k in E.KEYS:
            assert len(r[k + "_frames"]) == len(g[k + "_frames"])
            assert E.same(r[k], g[k], E.EMU_DISTANCE[k]).all(), (name, k, r[k], float(g[k]))
            assert E.same(r[k + "_frames"], g[k + "_frames"], E.EMU_DISTANCE[k]).all(), (name, k)
            ds, df = E.distance(r[k], g[k]), E.distance(r[k + "_frames"], g[k + "_frames"])
            worst[k] = max(worst[k], ds, df)
            row += "  %s %.2e / %.2e" % (k, ds, df)
        lines.append(row)
    path = os.environ.get("PDSE_METRICS_PARITY")
    if path:
        with open(path, "w") as f:
            f.write("numpy restatement of csrc/metrics.hip (tests/emu_metrics.py) against the reference's float64 results:\n"
                    "largest |difference| of the utterance score / of the per-frame values, per fixture\n")
            f.write("\n".join(lines) + "\n")
            for k in E.KEYS:
                f.write("%-9s largest distance %.2e  committed EMU_DISTANCE %.1e  tolerance (x10) %.1e\n"
                        % (k, worst[k], E.EMU_DISTANCE[k], E.TOL[k]))
    assert max(E.TOL.values()) < 1e-3


def test_fp32_spectral_stage_would_miss_four_decimals():
    """Why the kernel's spectral stage is float64: the same restatement with an fp32 spectral stage leaves single fwSNRseg
    frames more than 1e-3 dB from the reference (the measure squares the difference of two nearly equal band energies).
    PDSE_METRICS_PARITY=<file> appends the figures."""
    lines, worst = [], dict.fromkeys(("wss", "fwsnrseg"), 0.0)
    for name in ("snr0_L64000", "snr20_L160000", "silence_L32000"):
        g = E.load_case(name)
        r = E.emulate(*E.case_inputs(g), spectral=np.float32)
        row = "%-16s" % name
        for k in ("wss", "fwsnrseg"):
            ds, df = E.distance(r[k], g[k]), E.distance(r[k + "_frames"], g[k + "_frames"])
            far = float(np.mean(~E.same(r[k + "_frames"], g[k + "_frames"], 1e-3)))
            worst[k] = max(worst[k], df)
            row += "  %s %.2e / %.2e, frames beyond 1e-3: %.4f" % (k, ds, df, far)
        lines.append(row)
    assert worst["fwsnrseg"] > 1e-3
    path = os.environ.get("PDSE_METRICS_PARITY")
    if path:
        with open(path, "a") as f:
            f.write("\nthe same restatement with an fp32 spectral stage (fp32 tables, DFT, band energies, logs): score / per-frame "
                    "distance\n" + "\n".join(lines) + "\n")


def test_silence_and_identity_fixtures_say_what_the_tests_assume():
    g = E.load_case("silence_L32000")
    assert np.isnan(g["llr"]) and np.isfinite([g["ssnr"], g["wss"], g["fwsnrseg"]]).all()
    g = E.load_case("same_L4000")
    assert float(g["ssnr"]) == 35.0 and float(g["llr"]) == 0.0


def test_frame_counts_and_rounding_rule():
    M = pkg("metrics")
    for n in range(600, 2001):
        assert M.frame_count(n) == (n - 360) // 120 - 1 == int(n / 120 - 480 / 120)
    # Python's round is half to even: 0.95 * 10 = 9.5 -> 10, 0.95 * 30 = 28.5 -> 28, 0.95 * 50 = 47.5 -> 48 (the doubles are exact halves)
    assert [M.kept_count(m) for m in (1, 2, 10, 30, 50, 529)] == [1, 2, 10, 28, 48, 503]
    for m in range(1, 1400):
        assert M.kept_count(m) == int(np.rint(np.float64(m) * 0.95)) and 1 <= M.kept_count(m) <= m
    v = np.array([3.0, np.nan, 1.0, 2.0] * 5)
    assert E.trimmed_mean(v[:4]) != E.trimmed_mean(v[:4]) and E.trimmed_mean([1.0] * 19 + [np.nan]) == 1.0


def test_tables_are_what_the_kernels_assume():
    M, L = pkg("metrics"), pkg("_lib")
    t = M.tables()
    assert t.dtype == np.float64 and t.size == L.METRICS_TABLE_DOUBLES
    br = t[L.METRICS_OFF_BRANGE:L.METRICS_OFF_BRANGE + 50].reshape(25, 2)
    crit = t[L.METRICS_OFF_CRIT:L.METRICS_OFF_WEPS].reshape(25, 512)
    assert (br[:, 0] <= br[:, 1]).all() and br.max() < 256 and (crit[:, 256:] == 0).all()
    for i in range(25):
        assert crit[i, int(br[i, 0])] > 0 and crit[i, int(br[i, 1])] > 0 and crit[i, :int(br[i, 0])].sum() == 0
    text = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "pdse.h")).read()
    assert "#define PDSE_METRICS_OFF_BASIS %d" % L.METRICS_OFF_BASIS in text
    assert L.METRICS_OFF_CRIT == 512 + 480 * 1024 and L.METRICS_TABLE_DOUBLES == L.METRICS_OFF_BRANGE + 64


def test_composite_fixture():
    import torch

    M = pkg("metrics")
    tab = np.load(os.path.join(GOLDEN, "metrics_composite.npz"))["table"]
    for l, w, s, p, csig, cbak, covl in tab:
        got = M.composite(float(l), float(w), float(s), float(p))
        assert np.allclose(got, (csig, cbak, covl), rtol=0, atol=1e-12)
    t = [torch.tensor(tab[:, i]) for i in range(4)]
    got = M.composite(*t)
    assert all(torch.allclose(g, torch.tensor(tab[:, 4 + i]), rtol=0, atol=1e-12) for i, g in enumerate(got))


def test_argument_errors_need_no_device(lib):
    import ctypes as C

    with pytest.raises(lib.PdseError, match="metrics: null"):
        lib.launch(lib.MetricsDesc())
    buf = (C.c_double * 8)()
    ptr = C.addressof(buf)

    def desc(B, Lmax, lens):
        d = lib.MetricsDesc()
        host = (C.c_int32 * max(len(lens), 1))(*lens)
        d.clean = d.proc = d.lens = d.tables = d.frames = d.sorted = d.out = ptr
        d.lens_host = C.addressof(host)
        d.B, d.Lmax, d.Mmax = B, Lmax, (Lmax - 480) // 120
        d._keep = host
        return d

    with pytest.raises(lib.PdseError, match="metrics: B < 1"):
        lib.launch(desc(0, 4000, []))
    with pytest.raises(lib.PdseError, match="metrics: len < 600"):
        lib.launch(desc(2, 4000, [4000, 599]))
    with pytest.raises(lib.PdseError, match="metrics: len > Lmax"):
        lib.launch(desc(2, 4000, [4001, 4000]))
    assert lib.load().pdse_desc_size(lib.OP_METRICS) == C.sizeof(lib.MetricsDesc) and lib.ABI_VERSION == 9


def test_quality_rejects_bad_shapes_before_touching_a_device():
    import torch

    M = pkg("metrics")
    x = torch.zeros(2, 4000)
    with pytest.raises(ValueError):
        M.quality(x, torch.zeros(2, 3999))
    with pytest.raises(ValueError):
        M.quality(x[0], x[0])
    with pytest.raises(ValueError, match="two 480-sample frames"):
        M.quality(x, x, lens=[4000, 599])
    with pytest.raises(ValueError, match="longer than the batch"):
        M.quality(x, x, lens=[4000, 4001])
    with pytest.raises(ValueError):
        M.quality(x, x, lens=[4000])
    with pytest.raises(ValueError, match="two 480-sample frames"):
        M.quality(torch.zeros(1, 500), torch.zeros(1, 500))
    with pytest.raises(pkg("_lib").PdseError):
        M.quality(x, x)                      # valid arguments on the CPU: no fallback


def test_cli_pairs_sorted_files_and_asserts_equal_lengths(tmp_path):
    M, wavio = pkg("metrics"), pkg("wavio")
    ref, deg = tmp_path / "ref", tmp_path / "deg"
    ref.mkdir(), deg.mkdir()
    rs = np.random.RandomState(0)
    for name, n in (("b.wav", 1000), ("a.wav", 800), ("c.wav", 1000)):
        wavio.write_wav(str(ref / name), 0.1 * rs.standard_normal(n))
        wavio.write_wav(str(deg / name), 0.1 * rs.standard_normal(n))
    (ref / "notes.txt").write_text("not a wav")
    pairs = M.pair_files(str(ref), str(deg))
    assert [os.path.basename(r) for r, _ in pairs] == ["a.wav", "b.wav", "c.wav"]
    assert all(os.path.basename(r) == os.path.basename(g) for r, g in pairs)
    groups = M.load_pairs(pairs)
    assert sorted(groups) == [800, 1000] and len(groups[1000]) == 2 and groups[800][0][0].dtype == np.float32
    wavio.write_wav(str(deg / "c.wav"), 0.1 * rs.standard_normal(999))
    with pytest.raises(AssertionError, match="c.shape"):
        M.load_pairs(M.pair_files(str(ref), str(deg)))
    (deg / "d.wav").write_bytes((deg / "a.wav").read_bytes())
    with pytest.raises(AssertionError):
        M.pair_files(str(ref), str(deg))
    assert M.main([]) == 2
    empty = tmp_path / "empty"
    empty.mkdir()
    assert M.main([str(empty), str(empty)]) == 1          # a message, not a numpy error
