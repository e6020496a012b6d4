"""GPU tests of utterances in flight: ``ComplexDDPMTrainer.enhance_stream`` and ``generate_wav(inflight=)`` against the
one-at-a-time loop of an ``exclusive=False`` trainer (bit for bit, in order), the fallback of one item to "bf16x3", early close,
and the finiteness verdict of a ``SamplerPipeline(verdict=True)`` - clean, dirty, and replayed from its hipGraph."""
import argparse
import logging
import struct
import wave

import numpy as np
import pytest
import torch

from conftest import pkg, seeded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENGTHS = (1600, 2400, 1600, 3200, 2400, 1600, 1761)          # T = 11 .. 21; 1761 is no multiple of the hop
GIVEN = (1, 4, 6)                                              # items that bring their own x_T; the others draw it


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    lib = pkg("_lib")
    lib.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return lib


def _trainer(weights, out, prior="GCRN", ddpm_sd=None, **kw):
    ns = argparse.Namespace
    return pkg("trainer").ComplexDDPMTrainer(
        ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav=str(out)),
        ns(model=ns(name=prior), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
        device=DEV, prior_state_dict=weights(prior), ddpm_state_dict=weights("DiffUNet1") if ddpm_sd is None else ddpm_sd,
        exclusive=False, **kw)


def _seed(s):
    torch.manual_seed(s)
    torch.cuda.manual_seed_all(s)


def _items(lengths, given, B=1, seed=100):
    out = []
    for i, n in enumerate(lengths):
        wav = (seeded((B, n), seed + i) * (0.05 + 0.1 * i)).to(DEV)
        x_T = seeded((B, 2, 1 + n // 160, 161), seed + 50 + i).to(DEV) if i in given else None
        out.append((wav[0] if B == 1 and i % 2 else wav, x_T))      # 1-D and [1, L] alike
    return out


def _one_at_a_time(tr, items, seed):
    """What the loop over ``enhance`` gives: [(wav_out, spec)], the spectrogram taken from the plan that ran."""
    _seed(seed)
    out = []
    for wav, x_T in items:
        w = tr.enhance(wav if wav.dim() == 2 else wav[None], x_T=x_T)
        out.append((w, tr._pipes[next(reversed(tr._pipes))].spec.clone()))
    return out


def _same(got, want):
    assert len(got) == len(want)
    for i, ((gw, gs), (ww, ws)) in enumerate(zip(got, want)):
        assert gw.shape == ww.shape and gs.shape == ws.shape, i
        assert torch.equal(gw, ww) and torch.equal(gs, ws), i
        assert torch.isfinite(gw).all()


@pytest.fixture(scope="module")
def mixed(L, weights, tmp_path_factory):
    """The seven items, their one-at-a-time results under seed 5 and the generator state that loop leaves (computed once)."""
    items = _items(LENGTHS, GIVEN)
    want = _one_at_a_time(_trainer(weights, tmp_path_factory.mktemp("ref")), items, seed=5)
    return items, want, torch.cuda.get_rng_state(DEV)


@pytest.mark.parametrize("inflight", [3, 2])
def test_mixed_items_arrive_in_order_and_equal_the_loop(L, weights, tmp_path, mixed, inflight):
    """Seven B = 1 items of four lengths, some with their own x_T: every yielded pair equals the one-at-a-time result bit for bit,
    in item order, and the generator ends in the loop's state; a geometry a slot met twice was replayed from its hipGraph; a
    second stream on the same trainer gives the same."""
    items, want, state = mixed
    tr = _trainer(weights, tmp_path)
    _seed(5)
    got = list(tr.enhance_stream(iter(items), inflight=inflight))
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)
    _same(got, want)
    assert len(tr._slots) == inflight and all(len(s.pipes) <= tr.STREAM_PLANS <= tr.MAX_PLANS for s in tr._slots)
    pipes = [p for s in tr._slots for p in s.pipes.values()]
    assert all(p.verdict and p.split == "f16x2" for p in pipes)
    assert any(h >= 1 for s in tr._slots for h in s.hits.values())          # a slot met a geometry again: that pass was a graph replay
    assert not tr._range_fallback and not tr._streaming and not tr._pipes
    _seed(5)
    _same(list(tr.enhance_stream(items, inflight=inflight)), want)         # on the slots and plans the first stream left


def test_items_of_two_utterances(L, weights, tmp_path):
    items = _items((1600, 1600, 2400, 1600), (0, 3), B=2, seed=300)
    want = _one_at_a_time(_trainer(weights, tmp_path), items, seed=6)
    _seed(6)
    got = list(_trainer(weights, tmp_path).enhance_stream(items, inflight=2))
    assert got[0][0].shape == (2, 1600) and got[2][1].shape == (2, 2, 16, 161)
    _same(got, want)


def test_diffunet_prior(L, weights, tmp_path):
    items = _items((1600, 2400, 1600), (1,), seed=400)
    want = _one_at_a_time(_trainer(weights, tmp_path, prior="DiffUNet"), items, seed=7)
    _seed(7)
    _same(list(_trainer(weights, tmp_path, prior="DiffUNet").enhance_stream(items, inflight=3)), want)


def test_an_item_outside_the_window_is_repeated_on_bf16x3(L, weights, tmp_path, caplog):
    """Five items of one geometry, all with their own x_T; the third's x_T is 1e4 times a unit normal draw.  Encoder stage 1 of the
    eps-net scales its input by 2^PDSE_F16_ACT_EXP = 16 and splits it in registers (include/pdse.h), so every |x_T| above 0.41 of
    that item - two thirds of its elements - lies beyond 65504 / 16 = 4094: its hi planes are infinities (the case of
    test_gpu_f16x2.py's overflow test, reached through the input) and the pass ends non-finite.  On bf16 planes the same values
    are ordinary numbers.  Expected: the third result is the "bf16x3" trainer's, the others - items 4 and 5 were in flight when the
    verdict was read - are the f16x2 results; one warning; the geometry is in ``_range_fallback``."""
    items = [(w, seeded((1, 2, 11, 161), 550 + i).to(DEV) * (1.0e4 if i == 2 else 1.0)) for i, (w, _) in enumerate(_items((1600,) * 5, ()))]
    ref16 = _trainer(weights, tmp_path)
    want = _one_at_a_time(ref16, items[:2] + items[3:], seed=8)
    assert not ref16._range_fallback
    want.insert(2, _one_at_a_time(_trainer(weights, tmp_path, split="bf16x3"), items[2:3], seed=8)[0])
    assert all(torch.isfinite(w).all() and torch.isfinite(s).all() for w, s in want)
    tr = _trainer(weights, tmp_path)
    with caplog.at_level(logging.WARNING):
        got = list(tr.enhance_stream(items, inflight=3))
    _same(got, want)
    warned = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and "bf16x3" in warned[0].getMessage() and "fp16" in warned[0].getMessage()
    assert tr._range_fallback == {(1, None, 1600, False, True)}
    # the geometry stays on the fallback, in the stream and outside it
    again = list(tr.enhance_stream(items[2:4], inflight=2))
    assert torch.equal(again[0][0], want[2][0]) and not torch.equal(again[1][0], want[3][0])
    assert all(p.split == "bf16x3" for s in tr._slots for (k, _), p in s.pipes.items() if k[2] == 1600)
    assert torch.equal(tr.enhance(items[2][0], x_T=items[2][1]), want[2][0])
    # a trainer whose arithmetic has no window to leave has nothing to fall back to
    nan_item = (items[0][0], torch.full((1, 2, 11, 161), float("nan"), device=DEV))
    gen = _trainer(weights, tmp_path, split="bf16x3").enhance_stream([items[0], nan_item, items[1]], inflight=2)
    next(gen)
    with pytest.raises(L.PdseRangeError):
        next(gen)


def test_early_close_leaves_the_trainer_usable(L, weights, tmp_path, mixed):
    items, want, _ = mixed
    tr = _trainer(weights, tmp_path)
    _seed(5)
    gen = tr.enhance_stream(items[:5], inflight=3)
    got = [next(gen), next(gen)]
    with pytest.raises(RuntimeError, match="already"):
        next(tr.enhance_stream(items[:1], inflight=1))               # one stream per trainer at a time
    gen.close()
    _same(got, want[:2])
    assert not tr._streaming
    wav, x_T = items[1]
    out = tr.enhance(wav[None] if wav.dim() == 1 else wav, x_T=x_T)
    assert torch.equal(out, want[1][0])
    torch.cuda.synchronize()
    _same(list(tr.enhance_stream([items[1]], inflight=1)), want[1:2])


def test_streams_around_the_trainers_own_passes(L, weights, tmp_path, caplog):
    """A default (``exclusive=True``) trainer: a stream, then three one-at-a-time passes - whose plan is replayed from a hipGraph
    that holds the memset nodes of the persistent launches -, then the stream again, every slot replaying its graph.  With the
    verdict table cleared by a memset node the second stream read other data in its tables (seen at T = 401: every item came
    back flagged); the clear is a kernel.  Nothing is flagged, and the second stream's bits are the first's."""
    items = [(w, seeded((1, 2, 11, 161), 700 + i).to(DEV)) for i, (w, _) in enumerate(_items((1600,) * 6, (), seed=650))]
    ns = argparse.Namespace
    tr = pkg("trainer").ComplexDDPMTrainer(
        ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav=str(tmp_path)),
        ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
        device=DEV, prior_state_dict=weights("GCRN"), ddpm_state_dict=weights("DiffUNet1"))
    assert tr.exclusive
    with caplog.at_level(logging.WARNING):
        first = list(tr.enhance_stream(items, inflight=3))
        for w, x in items[:3]:
            tr.enhance(w if w.dim() == 2 else w[None], x_T=x)
        assert next(iter(tr._pipes.values())).plan.has_graph
        second = list(tr.enhance_stream(items, inflight=3))
        third = list(tr.enhance_stream(items, inflight=3))
    _same(second, first)
    _same(third, first)
    assert not tr._range_fallback and not [r for r in caplog.records if r.levelno >= logging.WARNING]
    for s in tr._slots:                                            # and the tables hold what the last pass counted: nothing
        for p in s.pipes.values():
            assert not p.verdict_tab.cpu().any()


def _write(path, samples, rate):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(samples.astype("<i2").tobytes())
    return str(path)


def test_file_loop_in_flight_writes_the_same_bytes(L, weights, tmp_path, caplog):
    """Five 16-bit files of three lengths at 16 and 48 kHz and a float file that is skipped: ``generate_wav(inflight=3)`` writes
    byte for byte what ``generate_wav(inflight=1)`` of an ``exclusive=False`` trainer writes under the same seed, and leaves the
    generator in the same state."""
    rs = np.random.RandomState(12)
    data = tmp_path / "noisy"
    data.mkdir()
    pcm = lambda n: (0.1 * 32768 * rs.standard_normal(n)).clip(-32768, 32767)   # noqa: E731
    _write(data / "a0.wav", pcm(1600), 16000)
    _write(data / "a1.wav", pcm(7200), 48000)                                   # 2400 samples at 16 kHz
    _write(data / "a2.wav", pcm(3200), 16000)
    _write(data / "a3.wav", pcm(4800), 48000)                                   # 1600
    raw = open(_write(data / "a4.wav", pcm(2400), 16000), "rb").read()
    (data / "a25_float.wav").write_bytes(raw[:20] + struct.pack("<H", 3) + raw[22:])     # WAVE_FORMAT_IEEE_FLOAT: rejected
    names = ["a0.wav", "a1.wav", "a2.wav", "a3.wav", "a4.wav"]
    runs = {}
    for inflight in (1, 3):
        tr = _trainer(weights, tmp_path / ("out%d" % inflight))
        _seed(41)
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            written = tr.generate_wav(load_pre_train=False, data_path=str(data), inflight=inflight)
        assert [w.split("/")[-1] for w in written] == names
        skipped = [r for r in caplog.records if "skipping" in r.getMessage()]
        assert len(skipped) == 1 and "a25_float.wav" in skipped[0].getMessage()
        runs[inflight] = ([open(w, "rb").read() for w in written], torch.cuda.get_rng_state(DEV))
    for a, b in zip(runs[1][0], runs[3][0]):
        assert len(a) >= 44 + 2 * 1600 and a == b
    assert len({len(a) for a in runs[1][0]}) == 3 and torch.equal(runs[1][1], runs[3][1])
    with pytest.raises(ValueError, match="batch"):
        tr.generate_wav(load_pre_train=False, data_path=str(data), batch=2, inflight=2)


def test_verdict_of_a_pipeline_clean_dirty_and_replayed(L, weights):
    """A ``verdict=True`` pipeline computes what one without it computes and reports (0, 0) on a clean pass; a NaN in x_T gives
    non-zero counts for the spectrogram and the waveform; a graph replay after a dirty pass reports the new pass only, because the
    clear is a launch of the plan."""
    P = pkg("pipeline").SamplerPipeline
    B, L_ = 1, 1600
    wav, x_T = seeded((B, L_), 61).to(DEV), seeded((B, 2, 11, 161), 62).to(DEV)
    bad = x_T.clone()
    bad[0, 1, 5, 80] = float("nan")
    plain = P(DEV, "GCRN", weights("GCRN"), weights("DiffUNet1"), B, L_=L_)
    pipe = P(DEV, "GCRN", weights("GCRN"), weights("DiffUNet1"), B, L_=L_, verdict=True)
    want = plain.enhance(wav, x_T)

    def counts():
        pipe.verdict_fetch()
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        return pipe.verdict_counts()

    got = pipe.enhance(wav, x_T)
    assert counts() == (0, 0) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    out = pipe.enhance(wav, bad)
    c = counts()
    assert c[0] > 0 and c[1] > 0
    assert c == (int((~torch.isfinite(out[1])).sum()), int((~torch.isfinite(out[0])).sum()))
    with pytest.raises(L.PdseRangeError):
        pipe.check()
    got = pipe.enhance(wav, x_T, graph=True)                                   # replay after a dirty pass: the new pass only
    assert counts() == (0, 0) and torch.equal(got[0], want[0])
    pipe.enhance(wav, bad, graph=True)
    assert counts() == c
    pipe.enhance(wav, x_T, graph=True)
    assert counts() == (0, 0)
    # a call that runs part of the plan is judged as well, from a cleared table (sample(): prior .. step0)
    spec_only = P(DEV, "GCRN", weights("GCRN"), weights("DiffUNet1"), B, T=11, verdict=True)
    feat = plain.feat.clone()
    spec_only.sample(feat, bad)
    spec_only.verdict_fetch()
    torch.cuda.synchronize()
    n1 = spec_only.verdict_counts()
    spec_only.sample(feat, x_T)
    spec_only.verdict_fetch()
    torch.cuda.synchronize()
    assert len(n1) == 1 and n1[0] > 0 and spec_only.verdict_counts() == (0,)
