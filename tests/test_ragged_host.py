"""CPU: the host side of exact ragged batches - the window / bucket planner of ``generate_wav(batch=N)``
(prior-diffuse_amd/raggedplan.py), the descriptors that carry the length tables, and the argument errors that need no device."""
import ctypes as C
import random

import pytest

from conftest import pkg


def test_windows_cover_the_paths_in_order():
    rp = pkg("raggedplan")
    assert rp.windows(0, 4) == []
    assert rp.windows(5, 4) == [(0, 5)]
    assert rp.windows(70, 4) == [(0, 32), (32, 64), (64, 70)]
    assert rp.windows(64, 32) == [(0, 64)] and rp.WINDOW_BATCHES == 8
    with pytest.raises(ValueError):
        rp.windows(3, 0)


def test_buckets_every_file_once_sorted_padded_and_deterministic():
    rp = pkg("raggedplan")
    rs = random.Random(7)
    lens = [rs.randint(161, 100000) for _ in range(37)] + [48000, 48000, 2560, 5120]
    for batch in (1, 2, 4, 32, 64):
        got = rp.buckets(lens, batch)
        flat = [i for idx, _ in got for i in idx]
        assert sorted(flat) == list(range(len(lens)))                               # every file exactly once
        assert [lens[i] for i in flat] == sorted(lens)                              # sorted by length across the buckets
        assert all(len(idx) == batch for idx, _ in got[:-1]) and 1 <= len(got[-1][0]) <= batch
        for idx, L_pad in got:
            assert L_pad % 2560 == 0 and L_pad >= max(lens[i] for i in idx) > L_pad - 2560
        assert got == rp.buckets(list(lens), batch)                                  # a function of the lengths alone
    a, b = lens.index(48000), lens.index(48000, lens.index(48000) + 1)
    flat = [i for idx, _ in rp.buckets(lens, 4) for i in idx]
    assert flat.index(a) + 1 == flat.index(b)                                        # equal lengths keep path order
    assert rp.padded_length(2560) == 2560 and rp.padded_length(2561) == 5120 and rp.padded_length(161) == 2560
    assert rp.padding_waste([2560] * 4, 4) == 1.0 and rp.padding_waste([2560, 5120], 2) == (2 * 33) / (17 + 33)


def test_draw_order_is_path_order_whatever_the_batch(monkeypatch, tmp_path):
    """The batched loop on a stubbed trainer: the generator is asked for the same shapes in the same order as the one-file loop
    asks for them (a draw per readable file in path order, each followed by its discards), and files are written in path order.
    Then ``generate_wav`` itself in its three modes - one file per pass, files in flight, ragged batches: the same draws, the
    same written paths and lengths in every mode, with and without the ``rng_fidelity`` discards."""
    import numpy as np
    import torch

    tr_mod = pkg("trainer")
    lens = {"a.wav": 4000, "b.wav": 161 + 160 * 7, "c.wav": None, "d.wav": 9000, "e.wav": 4000, "f.wav": 2000}
    calls, written, batches = [], [], []

    class Stub(tr_mod.ComplexDDPMTrainer):
        def __init__(self):
            self.prior_name, self.device = "GCRN", torch.device("cpu")
            self.params = pkg("params").params
            self.args = type("A", (), {"generated_wav": "out"})()

        def _load_window(self, paths):
            return [(p, torch.zeros(lens[p.split("/")[-1]])) for p in paths if lens[p.split("/")[-1]] is not None]

        def _x_T(self, shape, x_T):
            calls.append(("x_T", tuple(shape)))
            return torch.zeros(*shape)

        def _enhance_ragged(self, wavs, x_T, L_):
            batches.append(([w.numel() for w in wavs], L_))
            return [w.clone() for w in wavs]

        def enhance(self, wav, x_T=None, verify=True):
            return wav

        def enhance_stream(self, items, inflight=3):
            for wav, _ in items:
                yield wav, None

    monkeypatch.setattr(tr_mod.glob, "glob", lambda pat: ["d/" + k for k in reversed(sorted(lens))])
    monkeypatch.setattr(tr_mod.wavio, "write_wav", lambda dst, out, sr: written.append((dst, len(out))))
    monkeypatch.setattr(torch, "randn", lambda *shape, **kw: calls.append(("discard", tuple(shape))) or torch.zeros(1))
    tr = Stub()
    nd = len(tr.inference_schedule(tr.params.fast_sampling)[0]) - 1
    for batch in (2, 4):
        del calls[:], written[:], batches[:]
        out = tr._generate_wav_batched("d", True, batch)
        want = []
        for name in sorted(lens):
            if lens[name] is not None:
                shape = (1, 2, 1 + lens[name] // 160, 161)
                want += [("x_T", shape)] + [("discard", shape)] * nd
        assert calls == want
        assert [w[0] for w in written] == ["out/" + n for n in sorted(lens) if lens[n] is not None] == out
        assert [w[1] for w in written] == [lens[n] for n in sorted(lens) if lens[n] is not None]
        assert sorted(n for b, _ in batches for n in b) == sorted(v for v in lens.values() if v)
        assert all(L_ % 2560 == 0 and L_ >= max(b) and len(b) <= batch for b, L_ in batches)
    assert np.isfinite(nd) and nd >= 1
    tr.args.generated_wav = str(tmp_path)
    readable = [n for n in sorted(lens) if lens[n] is not None]
    for r in (True, False):
        want, seen = [], []
        for name in readable:
            shape = (1, 2, 1 + lens[name] // 160, 161)
            want += [("x_T", shape)] + [("discard", shape)] * (nd if r else 0)
        for b, i in ((1, 1), (1, 3), (2, 1), (4, 1)):
            del calls[:], written[:]
            out = tr.generate_wav(load_pre_train=False, data_path="d", rng_fidelity=r, batch=b, inflight=i)
            assert out == [w[0] for w in written]
            seen.append((list(calls), [w[0] for w in written], [w[1] for w in written]))
        assert all(s == seen[0] for s in seen)
        assert seen[0] == (want, [str(tmp_path / n) for n in readable], [lens[n] for n in readable])
        assert r or not any(c[0] == "discard" for c in seen[0][0])


def test_plan_cache_drops_the_least_recently_used_before_it_builds():
    """``_PlanCache`` alone, integers as plans: capacity 2 and takes of a, b, a, c, b."""
    cache = pkg("trainer")._PlanCache(2)
    built, alive = [], []

    def build(key):
        def make():
            alive.append(len(cache))                   # what is alive while the new plan is made
            built.append(key)
            return len(built)
        return make

    met = [cache.take(k, build(k))[1] for k in "abac"]
    assert met == [False, False, True, False] and built == ["a", "b", "c"]          # no build on the hit
    assert list(cache) == ["a", "c"] and cache["a"] == 1 and cache["c"] == 3      # b went, not a
    assert cache.hits == {"a": 1, "b": 0, "c": 0}
    plan, again = cache.take("b", build("b"))
    assert (plan, again) == (4, False) and built == ["a", "b", "c", "b"] and cache.hits["b"] == 0      # rebuilt: met_before False
    assert list(cache) == ["c", "b"]                                                # a went
    assert cache.take("b", build("b")) == (4, True) and cache.hits["b"] == 1 and len(built) == 4
    assert max(alive) < cache.capacity and len(cache) <= cache.capacity             # the eviction came before every build


def test_descriptors_match_the_library_after_the_new_fields():
    lib = pkg("_lib")
    so = lib.load()
    for kind in (lib.OP_WAVPREP, lib.OP_OLA, lib.OP_SIGMA, lib.OP_TCM, lib.OP_TCM2, lib.OP_TCM2S):
        assert so.pdse_desc_size(kind) == C.sizeof(lib.DESC_TYPES[kind]), lib.DESC_TYPES[kind].__name__
    # the tables are the LAST field of their descriptor and NULL in a fresh one: a dense caller sets nothing
    for typ, names in ((lib.WavprepDesc, ("reflect_own", "pad_")), (lib.OlaDesc, ("nframes", "lens")), (lib.SigmaDesc, ("valid",)),
                       (lib.TcmDesc, ("frames",)), (lib.Tcm2Desc, ("frames",))):
        assert tuple(n for n, _ in typ._fields_[-len(names):]) == names
        assert all(not getattr(typ(), n) for n in names)
    assert C.sizeof(lib.Tcm2sDesc) <= 4096                 # the stack descriptor travels as a kernel argument
    planfile = pkg("planfile")
    assert lib.Tcm2Desc.frames.offset in planfile.pointer_offsets(lib.Tcm2Desc)


def test_argument_errors_without_a_device():
    pl = pkg("pipeline")
    lens, frames = pl.ragged_tables([16000, 161, 3333], 3, 16000)
    assert lens.tolist() == [16000, 161, 3333] and frames.tolist() == [101, 2, 21] and str(lens.dtype) == str(frames.dtype) == "int32"
    assert pl.ragged_tables(4000, 2, 4000)[1].tolist() == [26, 26]
    for bad in ([16000, -5, 3333], [16000, 160, 3333], [16001, 400, 3333], [16000, 400]):
        with pytest.raises(ValueError):
            pl.ragged_tables(bad, 3, 16000)
    for prior in ("aia_complex_trans_ri", "dual_aia_trans_merge_crm"):
        with pytest.raises(ValueError, match="bidirectional GRU"):
            pl.ragged_args(prior, 16000)
        with pytest.raises(ValueError, match="bidirectional GRU"):
            pl.SamplerPipeline("cpu", prior, {}, {}, 2, L_=16000, ragged=True)
    with pytest.raises(ValueError, match="L_"):
        pl.SamplerPipeline("cpu", "GCRN", {}, {}, 2, T=20, ragged=True)
    pl.ragged_args("GCRN", 16000)
    pl.ragged_args("DiffUNet", 16000)
