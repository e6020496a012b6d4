"""GPU: exact ragged batches for the DB-AIAT priors (``ComplexDDPMTrainer(masked_prior=True)``,
``SamplerPipeline(ragged=True, masked_prior=True)``): the length-masked forms of the four operators that reach across frames -
attention, the bidirectional GRU, the GroupNorm statistics and the AHAM pool (csrc/aia.hip, csrc/gru3.hip) - and the whole
path on top of them.

Operators: a padded batch with a length table against the EXISTING dense launch on each item truncated to its own length;
``torch.equal`` on the own region, zeros (attention, GRU) or finite values (GroupNorm, AHAM) behind it.  Output buffers start
from a sentinel, and attention and GRU are launched a second time with the lengths permuted into the same buffers: what a
longer item left behind must not survive as anything but zeros.

Whole path: lengths (4000, 2500, 3300, 1121, 161) - T_b = 26, 16, 21, 8, 2 - on ``exclusive=False`` trainers, bit for bit
against each utterance through ``enhance`` alone; one utterance against the CPU oracle run alone at its own length (1e-4, the
suite's path tolerance; independent of this code base's dense kernels)."""
import argparse
import math
import os
import wave

import numpy as np
import pytest
import torch

from conftest import pkg, rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.678
AIA_PRIORS = ("aia_complex_trans_ri", "dual_aia_trans_merge_crm")
LENS = (4000, 2500, 3300, 1121, 161)
TOL = 1e-4


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    lib = pkg("_lib")
    lib.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return lib


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def _dev(t):
    return t.contiguous().to(DEV)


def _tab(lens):
    return torch.tensor(list(lens), dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------ attention
def _attn_desc(L, qd, out, E, axis, tab=None):
    B, _, T, F_ = qd.shape
    d = L.AttnDesc()
    d.qkv, d.out, d.B, d.T, d.F, d.E, d.heads, d.axis = qd.data_ptr(), out.data_ptr(), B, T, F_, E, 4, axis
    if tab is not None:
        d.seqlen = tab.data_ptr()
    return d


def _cut(t, axis, n):
    """The leading n positions of the sequence axis of a [B,C,T,F] tensor (axis 0: bins, axis 1: frames), contiguous."""
    return (t[:, :, :, :n] if axis == 0 else t[:, :, :n, :]).contiguous()


@pytest.mark.parametrize("kind", ["n01", "sharp"])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("E,lines,S,seqlen", [(32, 3, 65, (65, 4, 1)),              # a tail of the four-key grouping, a single key
                                              (64, 2, 1030, (1030, 513, 512))])     # either side of the 512-key image boundary
def test_attention_masked_equals_the_dense_launch_on_each_item_alone(L, E, lines, S, seqlen, axis, kind):
    B = len(seqlen)
    T, F_ = (lines, S) if axis == 0 else (S, lines)
    qkv = _randn(_gen(1300 + S + axis), B, 3 * E, T, F_)
    if kind == "sharp":
        qkv[:, :E] *= 30.0
    qd = _dev(qkv)
    out = torch.full((B, E, T, F_), SENTINEL, device=DEV)
    tab = _tab(seqlen)
    d = _attn_desc(L, qd, out, E, axis, tab)
    refs = {}

    def ref(b, n):
        if (b, n) not in refs:
            q1 = _cut(qd[b:b + 1], axis, n)
            o1 = torch.full((1, E) + tuple(q1.shape[2:]), SENTINEL, device=DEV)
            L.launch(_attn_desc(L, q1, o1, E, axis))
            torch.cuda.synchronize()
            refs[(b, n)] = o1
        return refs[(b, n)]

    for lens in (seqlen, seqlen[1:] + seqlen[:1]):      # the second launch: lengths permuted, same buffers
        tab.copy_(_tab(lens))
        L.launch(d)
        torch.cuda.synchronize()
        for b, n in enumerate(lens):
            own, behind = _cut(out[b:b + 1], axis, n), (out[b, :, :, n:] if axis == 0 else out[b, :, n:, :])
            assert torch.equal(own, ref(b, n)), (E, S, axis, kind, b, n)
            assert not behind.any(), (b, n, "queries behind the own length must store zeros")


# ------------------------------------------------------------------ bigru
FORMS = {"h64_fused": (64, True, 0), "h64_unfused": (64, False, 0), "h64_split": (64, True, 1), "h128_unfused": (128, False, 0)}


def _gru_weights(seed, H):
    g = _gen(seed)
    k = 1.0 / math.sqrt(H)

    def u(*shape):
        return (torch.rand(*shape, generator=g, dtype=torch.float32) * 2 - 1) * k

    return u(2, 3 * H, H // 2), u(2, 3 * H, H), u(2, 3 * H), u(2, 3 * H)


class _Gru:
    """The packed weights of one form (as the network plan packs them), and launches of it on given operands."""

    def __init__(self, L, form, W_ih, W_hh, b_ih, b_hh):
        P = pkg("packing")
        self.L, (self.H, self.fused, self.split) = L, FORMS[form]
        H = self.H

        def up(a, dtype=np.float32):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)

        def tiles(W, kin):
            return np.stack([np.stack([P.pack_s3_gather(W[dr, 32 * m:32 * m + 32].numpy().T, 1, kin)
                                       for m in range(3 * H // 32)], 0) for dr in range(2)], 0).view(np.int16)

        self.bhh, self.bih = up(b_hh.numpy()), up(b_ih.numpy())
        if self.split:
            self.whh, self.wih = up(tiles(W_hh, H), np.int16), up(tiles(W_ih, H // 2), np.int16)
        else:
            self.whh = up(np.stack([P.pack_a(W_hh[dr].numpy().T) for dr in range(2)], 0))
            self.wih = up(np.stack([P.pack_a(W_ih[dr].numpy().T) for dr in range(2)], 0)) if self.fused else None

    def desc(self, x, gx, y, tab=None):
        """x [B,H/2,T,F] and gx [B,6H,T,F] on the device (the form reads one of them); sequence along T (axis 1)."""
        B, _, T, F_ = x.shape
        d = self.L.GruDesc()
        d.y, d.B, d.T, d.F, d.H, d.axis, d.split = y.data_ptr(), B, T, F_, self.H, 1, self.split
        d.whh, d.bhh = self.whh.data_ptr(), self.bhh.data_ptr()
        if self.fused:
            d.x, d.wih, d.bih = x.data_ptr(), self.wih.data_ptr(), self.bih.data_ptr()
        else:
            d.gx = gx.data_ptr()
        if tab is not None:
            d.seqlen = tab.data_ptr()
        return d


@pytest.mark.parametrize("form", list(FORMS))
def test_bigru_masked_equals_the_dense_launch_on_each_item_alone(L, form):
    """33 lines of 11 per item: the first workgroup straddles all three items, the second holds one line."""
    B, T, F_, seqlen = 3, 7, 11, (7, 4, 1)
    H = FORMS[form][0]
    W_ih, W_hh, b_ih, b_hh = _gru_weights(1600, H)
    x = _randn(_gen(1601), B, H // 2, T, F_)
    gx = torch.cat([torch.einsum("gi,bitf->bgtf", W_ih[dr], x) + b_ih[dr].view(1, -1, 1, 1) for dr in range(2)], dim=1)
    gru = _Gru(L, form, W_ih, W_hh, b_ih, b_hh)
    xd, gxd = _dev(x), _dev(gx)
    y = torch.full((B, 2 * H, T, F_), SENTINEL, device=DEV)
    tab = _tab(seqlen)
    d = gru.desc(xd, gxd, y, tab)
    refs = {}

    def ref(b, n):
        if (b, n) not in refs:
            x1, g1 = xd[b:b + 1, :, :n].contiguous(), gxd[b:b + 1, :, :n].contiguous()
            y1 = torch.full((1, 2 * H, n, F_), SENTINEL, device=DEV)
            L.launch(gru.desc(x1, g1, y1))
            torch.cuda.synchronize()
            refs[(b, n)] = y1
        return refs[(b, n)]

    for lens in (seqlen, (1, 7, 4)):                    # the second launch: lengths permuted, same buffers
        tab.copy_(_tab(lens))
        L.launch(d)
        torch.cuda.synchronize()
        for b, n in enumerate(lens):
            r = ref(b, n)
            assert torch.equal(y[b, :H, :n], r[0, :H]), (form, "forward", b, n)
            assert torch.equal(y[b, H:, :n], r[0, H:]), (form, "backward", b, n)
            assert not y[b, :, n:].any(), (form, b, n, "positions behind the own length must store zeros")


# ------------------------------------------------------------------ gn_combine
GN_PARTS = 64


def _gn_desc(L, dev, stats, out, plane, B, C, k1, k2):
    d = L.GncombDesc()
    d.base, d.row, d.col, d.g_row, d.b_row, d.g_col, d.b_col = (t.data_ptr() for t in dev)
    d.stats, d.out, d.plane, d.B, d.C, d.k1, d.k2, d.eps = stats.data_ptr(), out.data_ptr(), plane, B, C, k1, k2, 1e-8
    return d


def test_gn_combine_masked_equals_the_dense_launch_on_each_item_alone(L):
    C, F_, T, frames = 32, 37, 9, (9, 5, 1)
    B = len(frames)
    g = _gen(1700)
    base = _randn(g, B, C, T, F_)
    row, col = _randn(g, B, C, T, F_) * 0.25 + 64.0, _randn(g, B, C, T, F_) * 0.25 + 64.0
    par = [1 + 0.3 * _randn(g, C), 0.2 * _randn(g, C), 0.8 + 0.3 * _randn(g, C), 0.2 * _randn(g, C)]
    k1, k2 = 0.7, -1.3
    dev = [_dev(t) for t in [base, row, col] + par]
    stats = torch.zeros(B, GN_PARTS, 4, device=DEV)
    out = torch.full((B, C, T, F_), SENTINEL, device=DEV)
    tab = _tab(frames)
    d = _gn_desc(L, dev, stats, out, T * F_, B, C, k1, k2)
    d.frames, d.per_frame = tab.data_ptr(), F_
    L.launch(d)
    torch.cuda.synchronize()
    for b, n in enumerate(frames):
        dev1 = [t[b:b + 1, :, :n].contiguous() for t in dev[:3]] + dev[3:]
        stats1 = torch.zeros(1, GN_PARTS, 4, device=DEV)
        out1 = torch.full((1, C, n, F_), SENTINEL, device=DEV)
        L.launch(_gn_desc(L, dev1, stats1, out1, n * F_, 1, C, k1, k2))
        torch.cuda.synchronize()
        assert torch.equal(stats[b], stats1[0]), (b, n)
        assert torch.equal(out[b, :, :n], out1[0]), (b, n)
        assert torch.isfinite(out[b]).all() and not (out[b] == SENTINEL).any(), (b, n, "finite values everywhere")
    # and the table is what makes the difference: the dense launch lets the padding frames into the moments
    outd = torch.empty_like(out)
    dd = _gn_desc(L, dev, stats, outd, T * F_, B, C, k1, k2)
    L.launch(dd)
    torch.cuda.synchronize()
    assert torch.equal(outd[0], out[0]) and not torch.equal(outd[1, :, :frames[1]], out[1, :, :frames[1]])


# ------------------------------------------------------------------ aham
def _aham_desc(L, xs, w, means, out, plane, B, C, bias):
    d = L.AhamDesc()
    for i in range(4):
        d.x[i] = xs[i].data_ptr()
    d.w, d.means, d.out, d.plane, d.B, d.C, d.bias = w.data_ptr(), means.data_ptr(), out.data_ptr(), plane, B, C, bias
    return d


def test_aham_masked_equals_the_dense_launch_on_each_item_alone(L):
    C, F_, T, frames = 64, 5, 51, (51, 20, 1)
    B = len(frames)
    g = _gen(1800)
    xs = [_dev(_randn(g, B, C, T, F_) + off) for off in (0.0, 3.0, -2.0, 6.0)]
    w, bias = _dev((torch.rand(C, generator=g) + 0.5) * 2.0 / C), 0.3
    means = torch.full((4, B, C), SENTINEL, device=DEV)
    out = torch.full((B, C, T, F_), SENTINEL, device=DEV)
    tab = _tab(frames)
    d = _aham_desc(L, xs, w, means, out, T * F_, B, C, bias)
    d.frames, d.per_frame = tab.data_ptr(), F_
    L.launch(d)
    torch.cuda.synchronize()
    for b, n in enumerate(frames):
        xs1 = [x[b:b + 1, :, :n].contiguous() for x in xs]
        means1 = torch.full((4, 1, C), SENTINEL, device=DEV)
        out1 = torch.full((1, C, n, F_), SENTINEL, device=DEV)
        L.launch(_aham_desc(L, xs1, w, means1, out1, n * F_, 1, C, bias))
        torch.cuda.synchronize()
        assert torch.equal(means[:, b], means1[:, 0]), (b, n)
        assert torch.equal(out[b, :, :n], out1[0]), (b, n)
        assert torch.isfinite(out[b]).all() and not (out[b] == SENTINEL).any(), (b, n, "finite values everywhere")


# ---------------------------------------------------------------------------------------------------------------------------
# whole path
# ---------------------------------------------------------------------------------------------------------------------------
def _trainer(weights, prior, out="y", **kw):
    ns = argparse.Namespace
    kw.setdefault("exclusive", False)
    return pkg("trainer").ComplexDDPMTrainer(
        ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav=out),
        ns(model=ns(name=prior), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
        device=DEV, prior_state_dict=weights(prior), ddpm_state_dict=weights("DiffUNet1"), **kw)


@pytest.fixture(scope="module")
def inputs():
    """Per-utterance waveforms (speech-like, different scales) and x_T at each utterance's own shape; never modified."""
    synth = pkg("synth")
    wavs = [torch.from_numpy(np.ascontiguousarray(synth.speechlike(1, n, 300 + i)[0])) * (0.5 + i) for i, n in enumerate(LENS)]
    g = torch.Generator().manual_seed(77)
    x_Ts = [torch.randn(2, 1 + n // 160, 161, generator=g, dtype=torch.float32) for n in LENS]
    return wavs, x_Ts


def _alone(tr, wavs, x_Ts):
    """Every utterance through the B = 1 path: [(wav [len], spec [2, T_b, 161])]."""
    out = []
    for w, x in zip(wavs, x_Ts):
        y = tr.enhance(w[None].to(DEV), x_T=x[None].to(DEV))[0].clone()
        out.append((y, tr._pipes[next(reversed(tr._pipes))].spec[0].clone()))
    return out


def _ragged_spec(tr):
    """The spectrogram of the last ragged pass as ``SamplerPipeline.enhance`` hands it out (frames behind T_b zeroed)."""
    pipe = tr._pipes[next(reversed(tr._pipes))]
    assert pipe.ragged and pipe.masked_prior
    spec = pipe.spec.clone()
    dead = torch.arange(pipe.T, device=DEV)[None, :] >= pipe.frames_tab[:, None]
    return spec.masked_fill_(dead[:, None, :, None], 0.0)


@pytest.mark.parametrize("split", ("f16x2", "bf16x3"))
@pytest.mark.parametrize("prior", AIA_PRIORS)
def test_whole_path_bit_identical_to_each_utterance_alone(L, weights, inputs, prior, split):
    """Fails on a trainer without the option (and on the code before it) with ValueError.  It also decides what reading could
    not: whether the 1x1 launches on frames-innermost operands add in an order that does not depend on the padded length."""
    wavs, x_Ts = inputs
    tr = _trainer(weights, prior, split=split, masked_prior=True)
    alone = _alone(tr, wavs, x_Ts)
    got = tr.enhance_batch(wavs, x_T=x_Ts, exact=True)
    pipe = tr._pipes[next(reversed(tr._pipes))]
    assert pipe.ragged and pipe.masked_prior and pipe.split == split and pipe.split_bf16
    spec = _ragged_spec(tr)
    for b, n in enumerate(LENS):
        Tb = 1 + n // 160
        assert got[b].shape == (n,)
        print(prior, split, n, "max |d wav|", float((got[b] - alone[b][0]).abs().max()),
              "max |d spec|", float((spec[b, :, :Tb] - alone[b][1]).abs().max()))
    for b, n in enumerate(LENS):
        Tb = 1 + n // 160
        assert torch.equal(got[b], alone[b][0]), (prior, split, n)
        assert torch.equal(spec[b, :, :Tb], alone[b][1]), (prior, split, n)
        assert not spec[b, :, Tb:].any()
    # the returned tensors of the pipeline itself: zeros behind an utterance's own samples and frames; finite intermediates
    batch = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True).to(DEV)
    batch = torch.nn.functional.pad(batch, (0, pipe.L - batch.shape[1]))
    xp = torch.zeros(len(LENS), 2, pipe.T, 161, device=DEV)
    for b, x in enumerate(x_Ts):
        xp[b, :, :x.shape[1]] = x.to(DEV)
    w2, s2 = pipe.enhance(batch, xp, lens=list(LENS), exact=True)
    pipe.check()
    for b, n in enumerate(LENS):
        assert torch.equal(w2[b, :n], alone[b][0]) and not w2[b, n:].any() and not s2[b, :, 1 + n // 160:].any()
    for t in (pipe.prior.att, pipe.prior.gy, pipe.prior.nxt, pipe.prior.merged, pipe.prior.out):
        assert torch.isfinite(t).all()


@pytest.mark.parametrize("prior", AIA_PRIORS)
def test_second_pass_with_permuted_lengths_and_graph_replay(L, weights, inputs, prior):
    wavs, x_Ts = inputs
    tr = _trainer(weights, prior, masked_prior=True)
    alone = _alone(tr, wavs, x_Ts)
    perm = [4, 3, 2, 1, 0]            # the shortest utterance sits where the longest was
    first = tr.enhance_batch(wavs, x_T=x_Ts, exact=True)
    pipe = tr._pipes[next(reversed(tr._pipes))]
    assert not pipe.plan.has_graph
    second = tr.enhance_batch([wavs[i] for i in perm], x_T=[x_Ts[i] for i in perm], exact=True)
    assert tr._pipes[next(reversed(tr._pipes))] is pipe and pipe.plan.has_graph          # same plan, now captured
    third = tr.enhance_batch(wavs, x_T=x_Ts, exact=True)                                  # a replay, lengths changed again
    for b in range(len(LENS)):
        assert torch.equal(first[b], alone[b][0]), b
        assert torch.equal(second[b], alone[perm[b]][0]), b
        assert torch.equal(third[b], alone[b][0]), b


def test_one_utterance_against_the_oracle_alone(L, weights, inputs):
    """aia_complex_trans_ri, the 3300-sample utterance of the batch against oracle/restate.py on that utterance alone."""
    from oracle import restate as R

    params = pkg("params").params
    prior, b = "aia_complex_trans_ri", LENS.index(3300)
    wavs, x_Ts = inputs
    tr = _trainer(weights, prior, masked_prior=True)
    got = tr.enhance_batch(wavs, x_T=x_Ts, exact=True)
    spec = _ragged_spec(tr)
    with torch.no_grad():
        ref_wav, ref_spec = R.enhance(prior, weights(prior), weights("DiffUNet1"), wavs[b][None], x_Ts[b][None],
                                      params.noise_schedule, params.inference_noise_schedule, True, False)
    Tb = 1 + LENS[b] // 160
    ew, es = rel_l2(got[b].cpu().numpy(), ref_wav[0].numpy()), rel_l2(spec[b, :, :Tb].cpu().numpy(), ref_spec[0].numpy())
    print(prior, LENS[b], "rel-L2 wav %.3e spec %.3e" % (ew, es))
    assert ew < TOL and es < TOL, (ew, es)


def _write_wav(path, x, rate):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


@pytest.mark.parametrize("prior", AIA_PRIORS)
def test_generate_wav_batched_writes_the_same_bytes(L, weights, tmp_path, prior):
    synth = pkg("synth")
    src = tmp_path / "in"
    src.mkdir()
    for i, n in enumerate((4000, 2900, 1777, 4000, 5300)):
        _write_wav(src / ("f%d.wav" % i), 0.5 * synth.speechlike(1, n, 60 + i)[0], 16000)
    outs = []
    for batch in (1, 3):
        tr = _trainer(weights, prior, out=str(tmp_path / ("out%d" % batch)), masked_prior=True)
        torch.manual_seed(4321)
        written = tr.generate_wav(load_pre_train=False, data_path=str(src), batch=batch)
        assert [os.path.basename(w) for w in written] == ["f%d.wav" % i for i in range(5)]
        outs.append(written)
    for one, three in zip(*outs):
        with open(one, "rb") as f1, open(three, "rb") as f3:
            assert f1.read() == f3.read(), os.path.basename(one)


@pytest.mark.parametrize("prior", AIA_PRIORS)
def test_a_default_trainer_still_refuses(L, weights, inputs, prior):
    wavs, _ = inputs
    tr = _trainer(weights, prior)
    assert tr.masked_prior is False
    with pytest.raises(ValueError, match="bidirectional GRU"):
        tr.enhance_batch([w[:3000] for w in wavs[:2]], exact=True)
    with pytest.raises(ValueError, match="bidirectional GRU"):
        tr.generate_wav(load_pre_train=False, data_path="nowhere", batch=2)
    with pytest.raises(ValueError, match="bidirectional GRU"):
        pkg("pipeline").SamplerPipeline(DEV, prior, weights(prior), weights("DiffUNet1"), 2, L_=2560, ragged=True)
