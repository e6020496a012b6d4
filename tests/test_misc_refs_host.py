"""CPU: (1) the statements of tests/helpers/misc_refs.py against torch's own modules in double - the GCRN tail against
ConvTranspose2d / BatchNorm2d (eval) / ELU / Linear, the step embedding against a TimeEmbedding assembled from the model's
text, wavprep against F.pad(reflect), the overlap-add against torch.istft with the periodic Hann window, the masked MSE
against utils/loss.py's expression; (2) every case of tests/helpers/misc_cases.py - the descriptors
tests/test_gpu_misc_ops.py launches - replayed on tests/emu.py and held to the float64 reference at 1e-6, with the NaN-margin
bookkeeping of the builder; (3) the packed Linear of the GCRN tail: emu.run_gcrnlast reads fcp, as the kernel does, and fcp
unpacks to fcT with zero rows behind input 160; (4) the 16419-row case still needs more tiles than the launch has workgroups."""
import numpy as np
import pytest
import torch
from torch import nn

import emu
from conftest import pkg, rel_l2
from helpers import misc_cases as G
from helpers import misc_refs as R

F32, F64 = torch.float32, torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ the references against torch
@pytest.mark.parametrize("bn", ["pos", "neg", "zero"])
def test_gcrn_tail_vs_torch_modules(bn):
    """model/gcrn.py:159-163 on torch's modules in double: d2 = elu(cat(a, e1)), d1 = elu(bn1_t(conv1_t(d2))), fc(d1)."""
    case = dict(id="host_" + bn, bn=bn)
    p = G.gcrn_params(case)
    g = _g(5)
    a = torch.randn(2, 16, 5, 80, generator=g, dtype=F64)
    e1 = torch.rand(2, 16, 5, 80, generator=g, dtype=F64) * 35 - 30
    conv1, conv2 = (nn.ConvTranspose2d(32, 1, (1, 3), stride=(1, 2)).double() for _ in range(2))
    bnm, fc, elu = nn.BatchNorm2d(1).double().eval(), nn.Linear(161, 161).double(), nn.ELU()
    with torch.no_grad():
        for m, w, b in ((conv1, "w1", "b1"), (conv2, "w2", "b2")):
            m.weight.copy_(p[w].double().reshape(32, 1, 1, 3))
            m.bias.fill_(float(np.float32(p[b])))
        bnm.weight.fill_(p["bn_w"]), bnm.bias.fill_(p["bn_b"]), bnm.running_mean.fill_(p["bn_mean"]), bnm.running_var.fill_(p["bn_var"])
        fc.weight.copy_(p["fc"].double()), fc.bias.copy_(p["fcb"].double())
        d2 = elu(torch.cat((a, e1), dim=1))
        want = fc(elu(bnm(conv1(d2) * torch.sigmoid(conv2(d2)))))[:, 0]
    got = R.gcrn_tail(elu(a), e1, p, F64)
    # the fold rounds scale and shift to fp32, as the descriptor carries them: 2^-24 relative on each
    assert rel_l2(got, want) < 2e-7
    sc, sh = pkg("packing").bn_fold(G.gcrn_state_dict(p), "bn1_t_2")
    assert (float(sc[0]), float(sh[0])) == R.bn_fold(p)
    if bn == "zero":
        assert R.bn_fold(p)[0] == 0.0
    if bn == "neg":
        assert R.bn_fold(p)[0] < 0.0


def test_time_embed_vs_model_text():
    class TimeEmbedding(nn.Module):
        def __init__(self, table):
            super().__init__()
            self.embedding = table
            self.projection1, self.projection2 = nn.Linear(128, 512), nn.Linear(512, 512)

        def forward(self, t):
            low_idx, high_idx = torch.floor(t).long(), torch.ceil(t).long()
            low, high = self.embedding[low_idx], self.embedding[high_idx]
            x = low + (high - low) * (t - low_idx).unsqueeze(1)
            x = self.projection1(x)
            x = x * torch.sigmoid(x)
            x = self.projection2(x)
            return x * torch.sigmoid(x)

    for ms in (50, 7):
        steps = torch.arange(ms).unsqueeze(1)
        table = steps * 10.0 ** (torch.arange(64).unsqueeze(0) * 4.0 / 63.0)
        table = torch.cat([torch.sin(table), torch.cos(table)], dim=1)
        assert torch.equal(R.time_table(ms), table) and table.dtype == F32
        case = dict(id="host_time", NF=37)
        p = G.time_params(case)
        m = TimeEmbedding(table.double()).double()
        fold = nn.Linear(512, 37).double()
        with torch.no_grad():
            m.projection1.weight.copy_(p["w1"]), m.projection1.bias.copy_(p["b1"])
            m.projection2.weight.copy_(p["w2"]), m.projection2.bias.copy_(p["b2"])
            fold.weight.copy_(p["wf"]), fold.bias.copy_(p["bf"])
            t = torch.tensor(G._tvals(ms), dtype=F32)
            want = m(t.double())
            temb, out = R.time_embed(t, table, p, F64)
            assert torch.allclose(temb, want, rtol=1e-12, atol=1e-13) and torch.allclose(out, fold(want), rtol=1e-12, atol=1e-13)
            t32, o32 = R.time_embed(t, table, p, F32)
        assert t32.dtype == F32 and rel_l2(t32, temb) < 1e-6 and rel_l2(o32, out) < 1e-6
        # an integral step is one table row exactly
        x_int = R.time_embed(torch.tensor([3.0]), table, dict(p, w1=torch.eye(512, 128), b1=torch.zeros(512)), F64)
        assert x_int[0].shape == (1, 512)


def test_wavprep_vs_torch_pad():
    x = torch.randn(3, 700, generator=_g(3), dtype=F64) * torch.tensor([0.05, 1.0, 20.0], dtype=F64)[:, None]
    xp, c = R.wavprep(x, 160, 1)
    want_c = torch.sqrt((x ** 2).sum(1) / 700)
    assert torch.allclose(c, want_c, rtol=1e-14)
    assert torch.allclose(xp, nn.functional.pad((x / want_c[:, None]).unsqueeze(1), (160, 160), mode="reflect")[:, 0], rtol=1e-14)
    xp, c = R.wavprep(x, 160, 0)
    assert bool((c == 1).all()) and torch.equal(xp, nn.functional.pad(x.unsqueeze(1), (160, 160), mode="reflect")[:, 0])
    # own: every utterance as if prepared alone, zeros behind
    lens = [161, 400, 700]
    xp, c = R.wavprep(x, 160, 1, lens, own=True)
    for b, n in enumerate(lens):
        one, c1 = R.wavprep(x[b:b + 1, :n], 160, 1)
        assert torch.equal(xp[b, :n + 320], one[0]) and not xp[b, n + 320:].any() and c[b] == c1[0]
    # lens alone: the RMS length only (0 clamps to 1)
    xp, c = R.wavprep(x, 160, 1, [0, 400, 900])
    assert torch.allclose(c, torch.stack([x[0, 0].abs(), torch.sqrt((x[1, :400] ** 2).mean()), want_c[2]]), rtol=1e-14)
    assert torch.allclose(xp[1], nn.functional.pad((x[1:2] / c[1]).unsqueeze(1), (160, 160), mode="reflect")[0, 0], rtol=1e-14)


@pytest.mark.parametrize("n_fft,hop,T,cut", [(320, 160, 9, 0), (320, 160, 3, 37), (10, 4, 7, 0), (8, 2, 9, 3)])
def test_ola_vs_torch_istft(n_fft, hop, T, cut):
    g = _g(n_fft + T)
    spec = torch.complex(torch.randn(2, n_fft // 2 + 1, T, generator=g, dtype=F64), torch.randn(2, n_fft // 2 + 1, T, generator=g, dtype=F64))
    spec[:, 0].imag.zero_(), spec[:, -1].imag.zero_()
    win = torch.hann_window(n_fft, periodic=True, dtype=F64)
    L = (T - 1) * hop - cut
    want = torch.istft(spec, n_fft, hop_length=hop, win_length=n_fft, window=win, length=L)
    frames = torch.fft.irfft(spec, n=n_fft, dim=1) * win[None, :, None]
    c = torch.tensor([0.7, 1.9], dtype=F64)
    got = R.ola(frames, win * win, n_fft, hop, L, c)
    assert torch.allclose(got, want * c[:, None], rtol=1e-10, atol=1e-12)
    # the ragged forms: an utterance that owns n frames and (n - 1) hop samples is the dense result of those frames
    n = T - 1
    if n >= 2:
        rag = R.ola(frames, win * win, n_fft, hop, L, None, nframes=[n, T + 5], lens=[(n - 1) * hop, L])
        alone = torch.istft(spec[:1, :, :n], n_fft, hop_length=hop, win_length=n_fft, window=win, length=(n - 1) * hop)
        assert torch.allclose(rag[0, :(n - 1) * hop], alone[0, :L], rtol=1e-10, atol=1e-12) and not rag[0, (n - 1) * hop:].any()
        assert torch.allclose(rag[1], want[1], rtol=1e-10, atol=1e-12)


def test_masked_mse_vs_loss_text():
    """utils/loss.py:34-44 as it stands (two channels, the longest utterance fills T)."""
    g = _g(11)
    esti, label = torch.randn(3, 2, 9, 161, generator=g, dtype=F64), torch.randn(3, 2, 9, 161, generator=g, dtype=F64)
    frame_list = [4, 9, 0]
    mask_for_loss = [torch.ones((f, esti.size()[-1]), dtype=esti.dtype) for f in frame_list]
    mask = nn.utils.rnn.pad_sequence(mask_for_loss, batch_first=True)
    com_mask = torch.stack((mask, mask), dim=1)
    want = float((((esti - label) * com_mask) ** 2).sum() / com_mask.sum())
    assert abs(R.masked_mse(esti, label, frame_list) - want) <= 1e-14 * want
    assert R.masked_mse(esti, label, [4, 14, -2]) == R.masked_mse(esti, label, frame_list)


# ------------------------------------------------------------------ the case tables on the emulator
def _replay(case):
    b = G.build(case, "cpu")
    emu.RUNNERS[type(b.desc)](b.desc, emu.Mem(G.tensors(b)))
    return b


def _close(got, want, what):
    w = torch.as_tensor(want)
    if w.numel():
        e = rel_l2(torch.as_tensor(got).double().numpy(), w.double().numpy())
        assert e <= 1e-6, (what, e)


def test_case_ids_are_unique():
    ids = G.by_id(G.ALL)
    assert len(set(ids)) == len(ids)


def test_big_gcrn_case_takes_a_second_trip():
    """More tiles than the launch has workgroups (csrc/misc.hip caps the grid), two workgroups with a second trip, a ragged tile."""
    import re

    src = open(pkg("_lib")._HERE + "/csrc/misc.hip").read()
    cap = int(re.search(r"gcrnlast_kernel, dim3\(ntiles < (\d+) \? ntiles : \1\)", src).group(1))
    assert cap == G.GCRN_GRID_CAP
    rows = G.GCRN_BIG["B"] * G.GCRN_BIG["T"]
    assert G.gcrn_ntiles(G.GCRN_BIG) > cap and G.gcrn_ntiles(G.GCRN_BIG) - cap == 2 and rows % 32 == 3
    assert all(G.gcrn_ntiles(c) <= cap for c in G.GCRN[:-1])


@pytest.mark.parametrize("case", G.GCRN, ids=G.by_id(G.GCRN))
def test_emulator_gcrnlast(case):
    b = _replay(case)
    B, T = case["B"], case["T"]
    assert b.desc.out_sb == 2 * T * 161 and b.desc.out == G.fptr(b.outbuf) + 4 * T * 161
    _close(G.read_plane(b.outbuf, B, T), b.ref(F64), case["id"])
    assert G.read_f(b.in0buf, (B, 16, T, 80)).equal(b.in0) and G.read_f(b.in1buf, (B, 16, T, 80)).equal(b.in1)


def test_gcrnlast_packed_matrix():
    """fcp, the only form of the matrix the kernel reads, holds fcT: rows 0 .. 160 equal, rows 161 .. 167 and columns 161 .. 191
    zero; and the emulator follows fcp, not fcT (a k-order error of the packer would show in every host replay)."""
    P = pkg("packing")
    b = G.build(G.find("gl_B3_T7"), "cpu")
    f = b.fields
    assert f["fcp"].shape == (6, 21, 64, 4) and f["fcp"].dtype == np.float32
    un = P.unpack_a4(f["fcp"], 6, 84)
    assert un.shape == (168, 192)
    assert np.array_equal(un[:161, :161], np.asarray(f["fcT"], np.float32)) and np.array_equal(f["fcT"], b.params["fc"].numpy().T)
    assert not un[161:].any() and not un[:, 161:].any()
    assert np.array_equal(f["w1"], b.params["w1"].numpy()) and np.array_equal(f["w2"], b.params["w2"].numpy())
    mem = emu.Mem(G.tensors(b))
    emu.run_gcrnlast(b.desc, mem)
    good = G.read_plane(b.outbuf, 3, 7)
    mem.arr(b.desc.fcT, 161 * 161)[:] = 0.0                      # not read
    emu.run_gcrnlast(b.desc, mem)
    assert G.read_plane(b.outbuf, 3, 7).equal(good)
    mem.arr(b.desc.fcp, 6 * 21 * 64 * 4).reshape(6, 21, 64, 4)[:, 9] = 0.0      # one kq group of every tile: inputs 72 .. 79
    emu.run_gcrnlast(b.desc, mem)
    assert rel_l2(G.read_plane(b.outbuf, 3, 7), b.ref(F64)) > 1e-2
    # the taps are told apart: main taps 0 and 2 exchanged
    b = G.build(G.find("gl_B3_T7"), "cpu")
    mem = emu.Mem(G.tensors(b))
    w1 = mem.arr(b.desc.w1, 96).reshape(32, 3)
    w1[:] = w1[:, ::-1].copy()
    emu.run_gcrnlast(b.desc, mem)
    assert rel_l2(G.read_plane(b.outbuf, 3, 7), b.ref(F64)) > 1e-2


@pytest.mark.parametrize("case", G.TIME + G.TIME_OOR, ids=G.by_id(G.TIME + G.TIME_OOR))
def test_emulator_time_embed(case):
    b = _replay(case)
    B, NF = case["B"], case["NF"]
    assert bool(b.desc.temb) == case["temb"] and bool(b.desc.wfT) == (NF > 0)
    ref = G.build(dict(case, t=case["clamped"]), "cpu").ref(F64) if "clamped" in case else b.ref(F64)
    _close(G.read_f(b.outbuf, (B, NF)), ref[1], case["id"] + " out")
    if case["temb"]:
        _close(G.read_f(b.tembbuf, (B, 512)), ref[0], case["id"] + " temb")
    else:
        assert G.untouched_f(b.tembbuf)


def test_time_cases_cover_the_issue():
    assert {c["NF"] for c in G.TIME} >= {0, 1, 64, 512, 513, 1000, 1024, 1500}
    assert {c["B"] for c in G.TIME} == {1, 3} and {c["ms"] for c in G.TIME} == {50, 7}
    assert any(c["NF"] > 0 and not c["temb"] for c in G.TIME) and any(c["NF"] == 0 and c["temb"] for c in G.TIME)
    for ms in (50, 7):
        used = {round(t, 6) for c in G.TIME if c["ms"] == ms for t in c["t"]}
        assert len(used) >= 5 and all(0 <= t <= ms - 1 for t in used)
    assert {round(t, 6) for c in G.TIME for t in c["t"] if c["ms"] == 50} == {round(t, 6) for t in G._tvals(50)}


@pytest.mark.parametrize("case", G.WAVPREP, ids=G.by_id(G.WAVPREP))
def test_emulator_wavprep(case):
    b = _replay(case)
    B, Lp = case["B"], case["L"] + 2 * case["pad"]
    xp, c = b.ref(F64)
    _close(G.read_f(b.xpadbuf, (B, Lp)), xp, case["id"] + " xpad")
    if case["c"]:
        _close(G.read_f(b.cbuf, (B,)), c, case["id"] + " c")
    else:
        assert G.untouched_f(b.cbuf)


@pytest.mark.parametrize("case", G.OLA, ids=G.by_id(G.OLA))
def test_emulator_ola(case):
    b = _replay(case)
    got = G.read_f(b.outbuf, (case["B"], case["L"]))
    _close(got, b.ref(F64), case["id"])
    if case["zero_w0"]:
        assert not got[:, 4::8].any() and bool((got[:, 5::8] != 0).all())


@pytest.mark.parametrize("case", G.MASKLOSS, ids=G.by_id(G.MASKLOSS))
def test_emulator_maskloss(case):
    b = _replay(case)
    L = pkg("_lib")
    got = float(G.read_f(b.outbuf, (1,))[0])
    want = b.ref()
    assert abs(got - want) <= 2e-6 * want
    part = G.read_d(b.partial, case["shape"][0] * L.MASKLOSS_BLOCKS).reshape(-1, L.MASKLOSS_BLOCKS)
    for i, f in enumerate(case["frames"]):
        assert (float(part[i].sum()) == 0.0) == (f <= 0)


def test_builder_margins():
    """The bookkeeping of the builder itself: pointers sit FM floats inside their allocations, outputs start as NaN throughout,
    inputs are NaN outside their extent - and where an utterance does not own them."""
    b = G.build(G.find("ola_320_T9_nframes"), "cpu")
    assert G.untouched_f(b.outbuf) and b.desc.out == b.outbuf.data_ptr() + 4 * G.FM
    fr = G_frames = b.framesbuf[G.FM:-G.FM].reshape(4, 320, 9)
    assert bool(torch.isnan(b.framesbuf[:G.FM]).all()) and bool(torch.isnan(b.framesbuf[-G.FM:]).all())
    assert bool(torch.isnan(fr[0]).all()) and bool(torch.isnan(fr[1, :, 1:]).all()) and bool(torch.isfinite(fr[1, :, 0]).all())
    assert bool(torch.isfinite(fr[2:]).all()) and G_frames.shape == b.frames.shape
    b = G.build(G.find("ml_3_2_9_161"), "cpu")
    e = b.estibuf[G.FM:-G.FM].reshape(3, 2, 9, 161)
    assert bool(torch.isnan(e[0]).all()) and bool(torch.isfinite(e[1:]).all()) and bool(torch.isnan(b.partial).all())
    b = G.build(G.find("gl_B1_T1"), "cpu")
    assert G.untouched_f(b.outbuf) and b.outbuf.numel() == 2 * 161 + 2 * G.FM
    for name in ("in0", "in1", "w1", "w2", "fcT", "fcp", "fcb", "out"):
        assert getattr(b.desc, name), name
    with pytest.raises(AssertionError):
        G.read_plane(b.outbuf, 1, 1)                             # nothing launched: nothing finite
    b = G.build(G.find("te_NF0_B1_ms50"), "cpu")
    assert b.outbuf.numel() == 2 * G.FM and not b.desc.wfT and not b.desc.bf and b.desc.out
