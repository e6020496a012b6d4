"""A plain torch statement of the recurrent core of the GCRN prior (the grouped LSTM: two layers of G = 2 independent
LSTMs of H = 512 units with LayerNorm(1024) behind each), in natural parameters - the state dict of the module itself:

    "lstm_list1.<g>.weight_ih_l0" [4H, H], ".weight_hh_l0" [4H, H], ".bias_ih_l0" [4H], ".bias_hh_l0" [4H]   (gate rows i, f, g, o)
    "lstm_list2.<g>. ..."  the same for layer 2,   "ln1.weight" / "ln1.bias" / "ln2.weight" / "ln2.bias" [G H]

    one cell:    c_t = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g),   h_t = sigmoid(o) tanh(c_t),   h_{-1} = c_{-1} = 0,
                 (i, f, g, o) = gx_t + W_hh h_{t-1},   gx_t = W_ih x_t + b_ih + b_hh
    layer 1:     group g reads chunk g of the input; the outputs are STACKED on a new last dim and flattened: feature 2 u + g
    LayerNorm 1  over those 1024 features (biased variance, eps inside the root)
    layer 2:     group g reads chunk g (features 512 g .. 512 g + 511) of LayerNorm 1's output; outputs CONCATENATED: 512 g + u

No packing, no fragment order, no folding of the LayerNorm into the projection.  Every function takes ``dtype``: float64
is the reference, the same functions at float32 are the fp32 CPU statement the tolerances are measured with.

Test infrastructure: held to torch.nn.LSTM / torch.nn.LayerNorm by tests/test_lstm_refs_host.py."""
import torch

G, H = 2, 512


def _t(v, dtype):
    return torch.as_tensor(v).to(dtype)


def project(x, p, layer, g, dtype=torch.float64):
    """gx = W_ih x + b_ih + b_hh of group g of ``layer`` ("lstm_list1" / "lstm_list2"): x [B, T, H] -> [B, T, 4H]."""
    k = "%s.%d." % (layer, g)
    return _t(x, dtype) @ _t(p[k + "weight_ih_l0"], dtype).T + (_t(p[k + "bias_ih_l0"], dtype) + _t(p[k + "bias_hh_l0"], dtype))


def layer(gx, whh, dtype=torch.float64):
    """One grouped layer from given input projections.  gx [G, B, T, 4H] (both biases included), whh: per group W_hh [4H, H]
    -> h [G, B, T, H]."""
    gx = _t(gx, dtype)
    ng, B, T, h4 = gx.shape
    n = h4 // 4
    out = torch.empty(ng, B, T, n, dtype=dtype)
    for g in range(ng):
        W = _t(whh[g], dtype).T.contiguous()
        h = torch.zeros(B, n, dtype=dtype)
        c = torch.zeros(B, n, dtype=dtype)
        for t in range(T):
            i_, f_, g_, o_ = torch.split(gx[g, :, t] + h @ W, n, dim=1)
            c = torch.sigmoid(f_) * c + torch.sigmoid(i_) * torch.tanh(g_)
            h = torch.sigmoid(o_) * torch.tanh(c)
            out[g, :, t] = h
    return out


def interleave(h):
    """[G, B, T, H] -> [B, T, G H], feature 2 u + g (stack on a new last dim, flatten)."""
    return torch.stack(list(h), dim=-1).flatten(-2)


def concat(h):
    """[G, B, T, H] -> [B, T, G H], feature 512 g + u."""
    return torch.cat(list(h), dim=-1)


def layernorm(x, gamma, beta, eps=1e-5, dtype=torch.float64):
    """Over the last dim: (x - mean) / sqrt(biased variance + eps) * gamma + beta."""
    x = _t(x, dtype)
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    return d / torch.sqrt(var + eps) * _t(gamma, dtype) + _t(beta, dtype)


def block(gx1, p, dtype=torch.float64, eps=1e-5, ln2=False):
    """Both layers with LayerNorm 1 between, from layer 1's input projections gx1 [G, B, T, 4H].
    Returns dict(y1 [B, T, 1024]: layer 1's output, interleaved, before LayerNorm 1;  y [B, T, 1024]: layer 2's output,
    concatenated; with ln2 also out: LayerNorm 2 of y)."""
    whh = lambda name: [p["%s.%d.weight_hh_l0" % (name, g)] for g in range(G)]      # noqa: E731
    y1 = interleave(layer(gx1, whh("lstm_list1"), dtype))
    z = layernorm(y1, p["ln1.weight"], p["ln1.bias"], eps, dtype)
    gx2 = torch.stack([project(c, p, "lstm_list2", g, dtype) for g, c in enumerate(torch.chunk(z, G, dim=-1))], 0)
    res = dict(y1=y1, y=concat(layer(gx2, whh("lstm_list2"), dtype)))
    if ln2:
        res["out"] = layernorm(res["y"], p["ln2.weight"], p["ln2.bias"], eps, dtype)
    return res


def ln_positions(B, T, N, osb, os_hi, os_lo, os_t, r, blk):
    """Where the strided, transposing store of pdse_ln_desc puts element j of row (b, t): int64 [B, T, N].
    c = j // r is a channel and j % r a position inside it; blk 8: channels live in blocks of 8."""
    b = torch.arange(B).view(B, 1, 1)
    t = torch.arange(T).view(1, T, 1)
    j = torch.arange(N).view(1, 1, N)
    c = torch.div(j, r, rounding_mode="floor")
    cpos = torch.div(c, 8, rounding_mode="floor") * os_hi + c % 8 if blk else c * os_hi
    return b * osb + cpos + (j % r) * os_lo + t * os_t


def ln_store(x, gamma, beta, size, strides, eps=1e-5, dtype=torch.float64):
    """LayerNorm over the last dim of x [B, T, N], scattered into a flat tensor of ``size`` elements (NaN where nothing is
    stored).  strides: dict(osb, os_hi, os_lo, os_t, r, blk)."""
    x = _t(x, dtype)
    out = torch.full((size,), float("nan"), dtype=dtype)
    pos = ln_positions(*x.shape, **strides)
    out[pos.reshape(-1)] = layernorm(x, gamma, beta, eps, dtype).reshape(-1)
    return out
