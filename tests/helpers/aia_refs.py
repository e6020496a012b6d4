"""Plain torch statements of the DB-AIAT operators of csrc/aia.hip / csrc/gru3.hip, in the kernels' own layouts
(include/pdse.h).  Every function computes in the dtype of its inputs: float64 inputs give the reference of
tests/test_gpu_aia_ops.py, float32 inputs the fp32 CPU evaluation its tolerances are derived from.  Nothing here
imports the package under test; tests/test_aia_refs_host.py holds these functions to torch's own modules in double."""
import torch


def rowln_prelu(x, gamma, beta, slope, eps=1e-5):
    """x [B,C,T,F]: LayerNorm over the F bins of every (b,c,t) row, then PReLU with the channel's slope [C]."""
    mean = x.mean(dim=-1, keepdim=True)
    e = x - mean
    var = (e * e).mean(dim=-1, keepdim=True)
    y = e / torch.sqrt(var + eps) * gamma + beta
    return torch.where(y > 0, y, slope.view(1, -1, 1, 1) * y)


def chln(x, gamma, beta, eps=1e-5):
    """x [B,C,plane]: LayerNorm over the C channels of every position."""
    mean = x.mean(dim=1, keepdim=True)
    e = x - mean
    var = (e * e).mean(dim=1, keepdim=True)
    return e / torch.sqrt(var + eps) * gamma.view(1, -1, 1) + beta.view(1, -1, 1)


def attention(qkv, E, axis, heads=4):
    """qkv [B,3E,T,F] (q already scaled by head_dim^-0.5) -> [B,E,T,F]: softmax(q k^T) v per (b, line, head);
    axis 0: the sequence runs over the bins F (one line per frame), axis 1: over the frames T.  Head h owns
    channels h E/heads .. (h+1) E/heads - 1."""
    B, _, T, F_ = qkv.shape
    hd = E // heads
    perm = (0, 3, 1, 4, 2) if axis == 0 else (0, 4, 1, 3, 2)          # -> [B, line, head, S, hd]
    q, k, v = (t.reshape(B, heads, hd, T, F_).permute(*perm) for t in qkv.split(E, dim=1))
    att = torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v
    back = (0, 2, 4, 1, 3) if axis == 0 else (0, 2, 4, 3, 1)          # -> [B, head, hd, T, F]
    return att.permute(*back).reshape(B, E, T, F_)


def _lines(t, axis):
    """[B,Cn,T,F] -> sequence-first [S, B * lines, Cn]."""
    B, Cn, T, F_ = t.shape
    if axis == 0:
        return t.permute(3, 0, 2, 1).reshape(F_, B * T, Cn)
    return t.permute(2, 0, 3, 1).reshape(T, B * F_, Cn)


def bigru(x, W_ih, W_hh, b_ih, b_hh, axis, gx=None):
    """Bidirectional single-layer GRU along one axis, zero initial state, gate order r, z, n:
        r = s(W_ir x + b_ir + W_hr h + b_hr), z likewise, n = tanh(W_in x + b_in + r (W_hn h + b_hn)), h' = (1-z) n + z h.
    x [B,I,T,F] with W_ih [2,3H,I] and b_ih [2,3H] - or, with gx given, gx [B,2*3H,T,F] = W_ih x + b_ih of both
    directions ([fw r,z,n | bw r,z,n]) and x, W_ih, b_ih unused.  W_hh [2,3H,H], b_hh [2,3H].
    Returns [B,2H,T,F] = [fw | bw]."""
    H = W_hh.shape[-1]
    src = gx if gx is not None else x
    B, _, T, F_ = src.shape
    seq = _lines(src, axis)                                           # [S, N, 6H] or [S, N, I]
    S, N, _ = seq.shape
    outs = []
    for d in range(2):
        g_in = seq[:, :, d * 3 * H:(d + 1) * 3 * H] if gx is not None else seq @ W_ih[d].T + b_ih[d]
        h = seq.new_zeros(N, H)
        ys = [None] * S
        for s in (range(S - 1, -1, -1) if d else range(S)):
            g_h = h @ W_hh[d].T + b_hh[d]
            r = torch.sigmoid(g_in[s, :, :H] + g_h[:, :H])
            z = torch.sigmoid(g_in[s, :, H:2 * H] + g_h[:, H:2 * H])
            n = torch.tanh(g_in[s, :, 2 * H:] + r * g_h[:, 2 * H:])
            h = (1 - z) * n + z * h
            ys[s] = h
        outs.append(torch.stack(ys, 0))
    y = torch.cat(outs, dim=-1)                                       # [S, N, 2H]
    if axis == 0:
        return y.reshape(F_, B, T, 2 * H).permute(1, 3, 2, 0).contiguous()
    return y.reshape(T, B, F_, 2 * H).permute(1, 3, 0, 2).contiguous()


def _gn1(x, gamma, beta, eps):
    """GroupNorm with one group on [B,C,plane]."""
    mean = x.mean(dim=(1, 2), keepdim=True)
    e = x - mean
    var = (e * e).mean(dim=(1, 2), keepdim=True)
    return e / torch.sqrt(var + eps) * gamma.view(1, -1, 1) + beta.view(1, -1, 1)


def gn_combine(base, row, col, g_row, b_row, g_col, b_col, k1, k2, eps=1e-8):
    """[B,C,plane] each: base + k1 GroupNorm(1,C)(row) + k2 GroupNorm(1,C)(col)."""
    return base + k1 * _gn1(row, g_row, b_row, eps) + k2 * _gn1(col, g_col, b_col, eps)


def aham(xs, w, bias):
    """xs: 4 layer outputs [B,C,plane]; w [C], bias: the 1x1 convolution on the pooled channels.
    out = x_3 + sum_i softmax_i(w . mean_plane(x_i) + bias) x_i."""
    y = torch.stack([(x.mean(dim=2) * w).sum(dim=1) + bias for x in xs], dim=1)      # [B,4]
    p = torch.softmax(y, dim=1)
    return xs[3] + sum(p[:, i].view(-1, 1, 1) * xs[i] for i in range(4))


def crm(mode, x, o=None, ri=None, a1=1.0, b1=0.0, a2=1.0, b2=0.0, a3=1.0, b3=0.0):
    """x [B,2,plane].  mode 0: |x| [B,plane].  mode 1: mask = s(a3 (s(a1 o + b1) tanh(a2 o + b2)) + b3) on o [B,plane],
    out [B,2,plane] = mask |x| (cos, sin)(atan2(im, re)) + ri."""
    re, im = x[:, 0], x[:, 1]
    mag = torch.sqrt(re * re + im * im)
    if mode == 0:
        return mag
    mask = torch.sigmoid(a3 * (torch.sigmoid(a1 * o + b1) * torch.tanh(a2 * o + b2)) + b3)
    ph = torch.atan2(im, re)
    return torch.stack((mask * mag * torch.cos(ph), mask * mag * torch.sin(ph)), dim=1) + ri
