"""Plain statements of what the small kernels of csrc/misc.hip compute, in a given dtype (float64: the reference; float32:
the same statement, whose distance from float64 is the e32 of the project's tolerance rule).  Written from the model's
text, not from the kernels; tests/test_misc_refs_host.py holds every one to torch's own modules on the CPU.

  gcrn_tail    model/gcrn.py:153-163: d2 = elu(cat(a, e1)); d1 = elu(bn1_t(conv1_t(d2))); out = fc(d1), with
               conv1_t = GluConvTranspose2d(32, 1, (1,3), stride (1,2)) and BatchNorm in eval mode, folded to one scale
               and one shift as packing.bn_fold folds it.  The operator takes in0 = elu(a) (its producer applied it) and
               in1 = e1 (the encoder's output: the concatenation's ELU is still to come).
  time_embed   model/diff3.py:62-95: the table, the lerp between two of its rows, two Linear + SiLU layers; then the
               folded per-stage biases, one more Linear on the embedding.
  wavprep      trainer/complex_ddpm_trainer.py:922-923 and torch.stft's centre padding: c = sqrt(sum x^2 / len),
               F.pad(x / c, reflect).  own=True: every utterance reflected at its own end, zeros behind the tail.
  ola          torch.istft (:1010-1016) behind the inverse DFT: overlap-add of windowed frames, division by the window
               envelope, the centre trim, the length cut and the rescale by c.
  masked_mse   utils/loss.py:34-44."""
import math

import numpy as np
import torch

BN_EPS = 1e-5


def _elu(x):
    return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0)))


def bn_fold(p):
    """Eval-mode BatchNorm of one channel -> (scale, shift), y * scale + shift, both rounded to fp32 as the descriptor
    carries them."""
    w, b, m, v = (float(np.float32(p[k])) for k in ("bn_w", "bn_b", "bn_mean", "bn_var"))      # fp32 parameters, folded in double
    scale = w / math.sqrt(v + BN_EPS)
    return float(np.float32(scale)), float(np.float32(b - m * scale))


def gcrn_tail(in0, in1, p, dtype=torch.float64):
    """in0, in1 [B,16,T,80]; p: w1, w2 [32,3] (input channel, tap), b1, b2, bn_w, bn_b, bn_mean, bn_var (scalars),
    fc [161,161] (out, in), fcb [161].  -> [B,T,161]."""
    c = lambda a: torch.as_tensor(a).to(dtype)                                            # noqa: E731
    u = torch.cat([c(in0), _elu(c(in1))], 1)                                              # d2 [B,32,T,80]
    B, C, T, Fi = u.shape
    W = torch.cat([c(p["w1"]).T, c(p["w2"]).T], 0)                                        # [6,32]: main taps 0..2, gate taps 0..2
    z = torch.matmul(W, u.reshape(B, C, T * Fi)).reshape(B, 6, T, Fi)
    pre = torch.zeros(B, 2, T, 2 * Fi + 1, dtype=dtype)
    for h in (0, 1):
        for k in range(3):                                                                # output bin 2 j + k <- input bin j
            pre[:, h, :, k:k + 2 * Fi:2] += z[:, 3 * h + k]
    y = (pre[:, 0] + float(np.float32(p["b1"]))) * torch.sigmoid(pre[:, 1] + float(np.float32(p["b2"])))
    scale, shift = bn_fold(p)
    y = _elu(y * scale + shift)
    return torch.matmul(y, c(p["fc"]).T) + c(p["fcb"])


def time_table(max_steps):
    """TimeEmbedding._build_embedding: float32 [max_steps,128]."""
    steps = torch.arange(max_steps).unsqueeze(1)
    dims = torch.arange(64).unsqueeze(0)
    table = steps * 10.0 ** (dims * 4.0 / 63.0)
    return torch.cat([torch.sin(table), torch.cos(table)], dim=1)


def _silu(x):
    return x * torch.sigmoid(x)


def time_embed(t, table, p, dtype=torch.float64):
    """t [B] inside [0, max_steps - 1]; p: w1 [512,128], b1, w2 [512,512], b2, wf [NF,512], bf [NF] (Linear layout: out, in).
    -> (temb [B,512], out [B,NF]).  float32: the products are added one by one in the order of the input index, as a
    thread of the kernel adds them."""
    c = lambda a: torch.as_tensor(a).to(dtype)                                            # noqa: E731
    t, table = c(t), c(table)
    low_idx, high_idx = torch.floor(t).long(), torch.ceil(t).long()
    low, high = table[low_idx], table[high_idx]
    x = low + (high - low) * (t - low_idx.to(dtype)).unsqueeze(1)

    def linear(x, w, b):
        w, b = c(w), c(b)
        if dtype == torch.float64:
            return x @ w.T + b
        s = b.unsqueeze(0).repeat(x.shape[0], 1)
        for i in range(w.shape[1]):
            s = s + x[:, i:i + 1] * w[:, i].unsqueeze(0)
        return s

    y = _silu(linear(x, p["w1"], p["b1"]))
    y = _silu(linear(y, p["w2"], p["b2"]))
    return y, linear(y, p["wf"], p["bf"])


def clamp_lens(lens, lo, hi):
    return [min(max(int(v), lo), hi) for v in lens]


def wavprep(x, pad, normalize, lens=None, own=False, dtype=torch.float64):
    """x [B,L] -> (xpad [B, L + 2 pad], c [B]).  lens: the samples an utterance owns (its RMS runs over them; counts outside
    [1, L] are clamped); own: reflected at its own end (at least pad + 1 samples), zeros behind the reflected tail."""
    x = torch.as_tensor(x).to(dtype)
    B, L = x.shape
    rms_len = clamp_lens(lens, 1, L) if lens is not None else [L] * B
    cs = torch.ones(B, dtype=dtype)
    if normalize:
        cs = torch.stack([torch.sqrt((x[b, :n] ** 2).sum() / n) for b, n in enumerate(rms_len)])
    out = torch.zeros(B, L + 2 * pad, dtype=dtype)
    for b in range(B):
        n = clamp_lens(lens, pad + 1, L)[b] if (own and lens is not None) else L
        row = (x[b, :n] / cs[b]).reshape(1, 1, n)
        out[b, :n + 2 * pad] = torch.nn.functional.pad(row, (pad, pad), mode="reflect").reshape(-1) if pad else row.reshape(-1)
    return out, cs


def ola(frames, win2, n_fft, hop, L, c=None, nframes=None, lens=None, dtype=torch.float64):
    """frames [B,n_fft,T], the windowed inverse transforms; win2 [n_fft], the squared window.  -> [B,L]: sample i is sample
    i + n_fft/2 of the overlap-add over the envelope (0 where no window reaches it), times c[b].  nframes: utterance b owns its
    first nframes[b] frames (clamped to [0, T]); lens: zeros from sample lens[b] on."""
    fr = torch.as_tensor(frames).to(dtype)
    w2 = torch.as_tensor(win2).to(dtype)
    B, _, T = fr.shape
    half = n_fft // 2
    full = max(n_fft + hop * (T - 1), half + L)
    out = torch.zeros(B, L, dtype=dtype)
    for b in range(B):
        y, env = torch.zeros(full, dtype=dtype), torch.zeros(full, dtype=dtype)
        Tb = T if nframes is None else min(max(int(nframes[b]), 0), T)
        for t in range(Tb):
            y[t * hop:t * hop + n_fft] += fr[b, :, t]
            env[t * hop:t * hop + n_fft] += w2
        y, env = y[half:half + L], env[half:half + L]
        ok = env > 1e-11
        v = torch.where(ok, y / torch.where(ok, env, torch.ones_like(env)), torch.zeros_like(y))
        if c is not None:
            v = v * torch.as_tensor(c).to(dtype)[b]
        if lens is not None:
            v[min(max(int(lens[b]), 0), L):] = 0
        out[b] = v
    return out


def masked_mse(esti, label, frames):
    """com_mse_loss on [B,C,T,F] in float64: ((esti - label) * mask) ** 2).sum() / mask.sum(), mask one on the first frames[b]
    frames (clamped to [0, T]) of every channel of utterance b."""
    e, l = torch.as_tensor(esti).double(), torch.as_tensor(label).double()
    B, C, T, F = e.shape
    mask = torch.zeros(B, C, T, F, dtype=torch.float64)
    for b, f in enumerate(frames):
        mask[b, :, :min(max(int(f), 0), T)] = 1.0
    d = torch.where(mask > 0, e - l, torch.zeros_like(e))        # a frame beyond an utterance's own is not read at all
    return float((d ** 2).sum() / mask.sum())
