"""A plain torch statement of what ONE launch of the eps-net block kernels computes (include/pdse.h: pdse_bglu_desc,
csrc/bglu.hip) - one encoder / decoder stage of the network behind its 1x1 input convolution, with the NEXT stage's 1x1
input convolutions chained onto it:

    encoder stage   h (conv1 output, 32 channels); one causal zero frame on top;
                    L = l(h), R = r(h)                      Conv2d (2, kw), stride (1, 2), kw = 5 (stage 1) or 3
                    G = L sigmoid(r_conv(R)) + R sigmoid(l_conv(L))
                    Y = PReLU(BatchNorm2d(conv2(G)))        32 -> 64, BatchNorm in eval mode
                    Z_i = W_i Y + bias_i[b]                 the next encoder stage's conv1 and the skip halves of both
                                                            decoders' conv1, every one with its own per-item bias
    stage 1         h itself from the two 2-channel inputs: u = Preprocess(cat(x, x_init)), one causal zero frame on top
                    of u, h = conv1(u) + bh[b] (bh: conv1's bias with the projected time embedding behind it, so the
                    pad frame of h is bh, not zero)
    decoder stage   the same with l / r as ConvTranspose2d (2, kw), stride (1, 2), the last frame chomped;
                    C2 = 64: Z_0 = W_0 Y + bias_0[b] + addend (the next decoder stage's conv1 over its first 64 input
                    channels plus the fp32 skip half the encoder left);  C2 = 1 (last stage): conv2 to one channel and
                    nothing else.
    decoder stage 5 conv1 alone: ``conv1_cat`` over cat(TCM output, encoder stage-5 output).

Natural parameters only (a dict per stage, see ``encoder`` / ``decoder``): convolution weights in torch's own layouts,
BatchNorm as (weight, bias, running_mean, running_var), the PReLU slope as a number.  Nothing is folded, packed or
re-ordered.

``rnd``: the one-plane form (np = 1) multiplies bf16 operands; round to bf16 (nearest even) at exactly the points at which
tests/emu.py: run_bglu does - the gather inputs, L / R in front of l_conv / r_conv (the gate multiplies the unrounded L /
R), G in front of conv2, Y in front of the chained tiles - and every MATRIX operand as the kernel holds it: the gather
weights (stage 1: the composition of l / r with conv1 and Preprocess, the only thing that can be rounded there), l_conv /
r_conv scaled by -log2 e, conv2 with the BatchNorm scale folded in, the chained weights.  Biases, the one-channel conv2 of
the last decoder stage (an fp32 dot product) and all arithmetic behind the products stay unrounded.  With ``rnd`` False
none of these foldings exists; tests/test_bglu_refs_host.py holds the two routes to each other with the rounding replaced
by the identity.

Test infrastructure: held to torch.nn's Conv2d / ConvTranspose2d / ConstantPad2d / BatchNorm2d / PReLU by
tests/test_bglu_refs_host.py."""
import torch
import torch.nn.functional as F

from helpers.tcm_refs import bf16

LOG2E = 1.4426950408889634
BN_EPS = 1e-5


def _t(v, dtype):
    return torch.as_tensor(v).to(dtype)


def _item(v, dtype):
    """[B or 1, C] (or [C]) -> [B or 1, C, 1, 1]."""
    v = _t(v, dtype)
    return v.reshape((1,) * (2 - v.dim()) + tuple(v.shape) + (1, 1))


def _c1(W, x):
    return torch.einsum("oc,bctf->botf", W, x)


def _prelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def _wq(W, fold, q):
    """The matrix [out, in] as the kernel's operand carries it: q(fold[o] W[o, :]) / fold[o] (fold 0: the product is zero
    either way); q None: W."""
    if q is None:
        return W
    fold = torch.as_tensor(fold, dtype=W.dtype).expand(W.shape[0])[:, None]
    safe = torch.where(fold != 0, fold, torch.ones_like(fold))
    return torch.where(fold != 0, q(W * fold) / safe, W)


def bn_scale(bn, dtype):
    w, _, _, var = (_t(v, dtype) for v in bn)
    return w / torch.sqrt(var + BN_EPS)


def tail(L, R, p, dtype=torch.float64, rnd=False, add=None, q=None):
    """Everything behind the two gather convolutions.  -> dict(L, R, G[, Y, Z (list)] or [, out])."""
    q = q if q is not None else (bf16 if rnd else None)
    rq = q if q is not None else (lambda v: v)
    Wlc, Wrc = _wq(_t(p["Wlc"], dtype), -LOG2E, q), _wq(_t(p["Wrc"], dtype), -LOG2E, q)
    mL = _c1(Wlc, rq(L)) + _item(p["blc"], dtype)
    mR = _c1(Wrc, rq(R)) + _item(p["brc"], dtype)
    G = L * torch.sigmoid(mR) + R * torch.sigmoid(mL)
    out = dict(L=L, R=R, G=G)
    W2 = _t(p["W2"], dtype)
    if W2.shape[0] == 1:                                   # the last decoder stage: one channel, no BatchNorm, no PReLU
        out["out"] = _c1(W2, G)[:, 0] + _t(p["b2"], dtype)[0]
        return out
    w, b, mean, var = (_t(v, dtype).view(1, -1, 1, 1) for v in p["bn"])
    O = _c1(_wq(W2, bn_scale(p["bn"], dtype), q), rq(G)) + _item(p["b2"], dtype)
    Y = _prelu((O - mean) / torch.sqrt(var + BN_EPS) * w + b, float(p["slope"]))
    out["Y"] = Y
    Z = []
    for i, tl in enumerate(p.get("nx", ())):
        z = _c1(_wq(_t(tl["W"], dtype), 1.0, q), rq(Y)) + _item(tl["bias"], dtype)
        if i == 0 and add is not None:
            z = z + add.to(dtype)
        Z.append(z)
    out["Z"] = Z
    return out


def stage1_h(x0, x1, p, dtype=torch.float64):
    """[B, 32, T + 1, F]: conv1 of the padded Preprocess output, per-item bias bh."""
    u = _c1(_t(p["Wpre"], dtype), torch.cat([x0, x1], 1).to(dtype)) + _item(p["bpre"], dtype)
    return _c1(_t(p["W1"], dtype), F.pad(u, (0, 0, 1, 0))) + _item(p["bh"], dtype)


def encoder(p, dtype=torch.float64, h=None, x0=None, x1=None, rnd=False, q=None):
    """p: Wl, Wr [32, 32, 2, kw] (Conv2d), bl, br [B or 1, 32], Wlc, Wrc [32, 32] (out, in), blc, brc [32], W2 [64, 32], b2,
    bn, slope, nx: [dict(W [32, 64], bias [B or 1, 32])]; stage 1 (h None): Wpre [2, 4], bpre, W1 [32, 2], bh [B or 1, 32]."""
    q = q if q is not None else (bf16 if rnd else None)
    Wl, Wr = _t(p["Wl"], dtype), _t(p["Wr"], dtype)
    if h is not None:
        hp = F.pad(h.to(dtype), (0, 0, 1, 0))
        if q is not None:
            hp, Wl, Wr = q(hp), q(Wl), q(Wr)
        L, R = F.conv2d(hp, Wl, stride=(1, 2)), F.conv2d(hp, Wr, stride=(1, 2))
    elif q is None:
        hp = stage1_h(x0, x1, p, dtype)
        L, R = F.conv2d(hp, Wl, stride=(1, 2)), F.conv2d(hp, Wr, stride=(1, 2))
    else:
        # l(h) = l(W1 Wpre x4) + l(c): the part the kernel multiplies (bf16 inputs, bf16 composed weights) and the part it
        # receives as biases (c: h of a zero input - bh on the pad frame, W1 bpre + bh below it)
        x4 = F.pad(torch.cat([x0, x1], 1).to(dtype), (0, 0, 1, 0))
        A = _t(p["W1"], dtype) @ _t(p["Wpre"], dtype)
        c = stage1_h(torch.zeros_like(x0), torch.zeros_like(x1), p, dtype)
        L, R = (F.conv2d(q(x4), q(torch.einsum("ockf,ci->oikf", W, A)), stride=(1, 2)) + F.conv2d(c, W, stride=(1, 2)) for W in (Wl, Wr))
    return tail(L + _item(p["bl"], dtype), R + _item(p["br"], dtype), p, dtype, rnd, q=q)


def decoder(p, h, dtype=torch.float64, rnd=False, add=None, q=None):
    """p as for ``encoder`` with Wl, Wr [32 in, 32 out, 2, kw] (ConvTranspose2d) and W2 [C2, 32] (out, in), C2 64 or 1;
    add: the fp32 skip addend of chained tile 0, [B, 32, T, Fo]."""
    q = q if q is not None else (bf16 if rnd else None)
    h, Wl, Wr = h.to(dtype), _t(p["Wl"], dtype), _t(p["Wr"], dtype)
    if q is not None:
        h, Wl, Wr = q(h), q(Wl), q(Wr)
    T = h.shape[2]
    L = F.conv_transpose2d(h, Wl, stride=(1, 2))[:, :, :T] + _item(p["bl"], dtype)
    R = F.conv_transpose2d(h, Wr, stride=(1, 2))[:, :, :T] + _item(p["br"], dtype)
    return tail(L, R, p, dtype, rnd, add, q=q)


def conv1_cat(xs, Ws, biases, dtype=torch.float64):
    """Decoder stage 5's conv1 over cat(xs) (TCM output[, encoder stage-5 output]; [B, C, T, F]) for every weight set of Ws
    ([32, C0 + C1], out x in) with per-item biases [B or 1, 32] (None: none) -> list of [B, 32, T, F]."""
    x = torch.cat([v.to(dtype) for v in xs], 1)
    return [_c1(_t(W, dtype), x) + (0 if b is None else _item(b, dtype)) for W, b in zip(Ws, biases)]
