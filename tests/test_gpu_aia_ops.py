"""Operator-level parity of the DB-AIAT kernels (csrc/aia.hip, csrc/gru3.hip) through the C-ABI: every kernel alone
against a plain float64 statement of its operation (tests/helpers/aia_refs.py, held to torch's own modules by
tests/test_aia_refs_host.py), at the shapes where its code takes another path - tails, masks, chunks, thresholds.

Tolerance, the same rule for every case: the operation is also evaluated with torch in fp32 on the CPU,
    e32 = rel_l2(fp32 CPU, float64),        rel_l2(kernel, float64) <= max(4 * e32, 2e-6).
The factor 4 covers the hardware exp2 / rcp against libm and another summation order; 2e-6 is the bound the attention
core is held to elsewhere in this suite.  Neither e32 nor the reference comes from the code under test.  Measured
values: profiles/aia_ops_margins.txt (PDSE_MARGINS)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import pkg, rel_l2
from helpers import aia_refs as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DISTS = {"n01": (0.0, 1.0), "m8": (8.0, 1.0), "m64": (64.0, 0.25)}


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


def _d(*ts):
    return [t.double() for t in ts]


def _check(got, ref64, ref32):
    """The tolerance rule of this file.  got: kernel result, ref64: float64 reference, ref32: torch fp32 on the CPU."""
    ref64 = ref64.numpy()
    err = rel_l2(got.cpu().numpy(), ref64)
    e32 = rel_l2(ref32.numpy(), ref64)
    bound = max(4 * e32, 2e-6)
    print("kernel %.3e  fp32 cpu %.3e  bound %.3e  kernel/e32 %.2f" % (err, e32, bound, err / e32 if e32 else math.inf))
    assert np.isfinite(err) and err <= bound, (err, e32, bound)


# ------------------------------------------------------------------ transpose
@pytest.mark.parametrize("N,R,Cc", [(3, 1, 1), (2, 31, 33), (2, 33, 31), (1, 64, 32), (2, 401, 80), (1, 80, 1001)])
def test_transpose_bit_exact(L, N, R, Cc):
    x = _randn(_gen(1), N, R, Cc)
    xd, out = _dev(x), torch.full((N, Cc, R), -7.0, device=DEV)
    d = L.TransposeDesc()
    d.in_, d.out, d.N, d.R, d.Cc = xd.data_ptr(), out.data_ptr(), N, R, Cc
    L.launch(d)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), x.permute(0, 2, 1).contiguous())


# ------------------------------------------------------------------ rowln_prelu
SENTINEL = -12345.678
ROWLN_F = [36, 64, 65, 80, 161, 192]


def _rowln_desc(L, x, gamma, beta, slope, out, out_sb):
    B, C, T, F_ = x.shape
    d = L.RowlnDesc()
    d.in_, d.gamma, d.beta, d.slope, d.out = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), slope.data_ptr(), out.data_ptr()
    d.out_sb, d.B, d.C, d.T, d.F, d.eps = out_sb, B, C, T, F_, 1e-5
    return d


@pytest.mark.parametrize("dist", ["n01", "m64"])
@pytest.mark.parametrize("B,C,T", [(1, 3, 5), (1, 1, 17), (2, 3, 3)])        # 15, 17, 18 rows: tails of the 16-row block
@pytest.mark.parametrize("F_", ROWLN_F)
def test_rowln_prelu(L, F_, B, C, T, dist):
    g = _gen(100 + F_)
    mean, std = DISTS[dist]
    x = _randn(g, B, C, T, F_) * std + mean
    gamma, beta = 1 + 0.3 * _randn(g, F_), 0.2 * _randn(g, F_)
    k = ROWLN_F.index(F_) % 3                                                 # negative, zero and > 1, rotated with F so that
    slope = torch.tensor(([-0.5, 0.0, 1.7] * 2)[k:k + C])                     # the one-channel shape meets each class too
    n = C * T * F_
    out = torch.full((B, 2 * n), SENTINEL, device=DEV)                        # items sit 2 n apart in a wider buffer
    xd, gd, bd, sd = _dev(x), _dev(gamma), _dev(beta), _dev(slope)
    L.launch(_rowln_desc(L, xd, gd, bd, sd, out, 2 * n))
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.equal(out[:, n:], torch.full((B, n), SENTINEL)), "wrote between the items"
    ref64 = A.rowln_prelu(*_d(x, gamma, beta, slope), 1e-5)
    ref32 = F.prelu(F.layer_norm(x, (F_,), gamma, beta, 1e-5), slope)
    _check(out[:, :n].reshape(B, C, T, F_), ref64, ref32)


def test_rowln_refuses_193_bins(L):
    x, v = torch.zeros(1, 1, 1, 193, device=DEV), torch.zeros(193, device=DEV)
    out = torch.full((193,), SENTINEL, device=DEV)
    with pytest.raises(L.PdseError, match="F <= 192"):
        L.launch(_rowln_desc(L, x, v, v, v, out, 193))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((193,), SENTINEL)), "a refused descriptor launched"


# ------------------------------------------------------------------ chln
def _chln_desc(L, x, gamma, beta, out):
    B, C, plane = x.shape
    d = L.ChlnDesc()
    d.in_, d.gamma, d.beta, d.out = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr()
    d.plane, d.B, d.C, d.eps = plane, B, C, 1e-5
    return d


@pytest.mark.parametrize("dist", ["n01", "m64"])
@pytest.mark.parametrize("plane", [1, 255, 257])
@pytest.mark.parametrize("C", [1, 16, 32, 64])
def test_chln(L, C, plane, dist):
    g = _gen(200 + C)
    mean, std = DISTS[dist]
    B = 2
    x = _randn(g, B, C, plane) * std + mean
    gamma, beta = 1 + 0.3 * _randn(g, C), 0.2 * _randn(g, C)
    xd, gd, bd = _dev(x), _dev(gamma), _dev(beta)
    out = torch.full((B, C, plane), SENTINEL, device=DEV)
    L.launch(_chln_desc(L, xd, gd, bd, out))
    torch.cuda.synchronize()
    ref64 = A.chln(*_d(x, gamma, beta), 1e-5)
    ref32 = F.layer_norm(x.permute(0, 2, 1), (C,), gamma, beta, 1e-5).permute(0, 2, 1)
    _check(out, ref64, ref32)


def test_chln_refuses_65_channels(L):
    x, v = torch.zeros(1, 65, 4, device=DEV), torch.zeros(65, device=DEV)
    out = torch.full((1, 65, 4), SENTINEL, device=DEV)
    with pytest.raises(L.PdseError, match="C <= 64"):
        L.launch(_chln_desc(L, x, v, v, out))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.full((1, 65, 4), SENTINEL)), "a refused descriptor launched"


# ------------------------------------------------------------------ attention
def _attention(L, qkv, E, axis):
    B, _, T, F_ = qkv.shape
    qd = _dev(qkv)
    out = torch.full((B, E, T, F_), SENTINEL, device=DEV)
    d = L.AttnDesc()
    d.qkv, d.out, d.B, d.T, d.F, d.E, d.heads, d.axis = qd.data_ptr(), out.data_ptr(), B, T, F_, E, 4, axis
    L.launch(d)
    torch.cuda.synchronize()
    return out


def _qkv(seed, B, E, S, lines, axis, kind):
    """kind 'n01': N(0,1); 'sharp': q scaled by 30 - the softmax is near one-hot, so the online rescale and the
    m = -1e30 start carry the result; 'flat': every key of a line equal - uniform weights, the output is the mean of v."""
    T, F_ = (lines, S) if axis == 0 else (S, lines)
    qkv = _randn(_gen(seed), B, 3 * E, T, F_)
    if kind == "sharp":
        qkv[:, :E] *= 30.0
    if kind == "flat":
        k = qkv[:, E:2 * E]
        qkv[:, E:2 * E] = (k[:, :, :, :1] if axis == 0 else k[:, :, :1, :]).clone().expand_as(k)
    return qkv


# Which path a case takes follows from the launcher's LDS budget: one image of a head's K and V is 2 S (E / 4) floats and
# may take 64 KB, so it holds up to ATTN_CAP[E] keys; a longer line is walked in key chunks of ATTN_CAP[E] keys, every
# chunk but the last a multiple of four.  A workgroup has at most 1024 threads, one query each: a line of more
# positions takes several query rounds - and, since 1024 >= ATTN_CAP[E], always the chunked path.
ATTN_CAP = {32: 1024, 64: 512}


def _attn_case(L, seed, B, E, S, lines, axis, kind):
    n = (S + ATTN_CAP[E] - 1) // ATTN_CAP[E]
    print("E %d S %d: %s, last of %d keys; %d query round(s)" % (E, S, "one image" if n == 1 else "%d key chunks" % n,
                                                                S - (n - 1) * ATTN_CAP[E], (S + 1023) // 1024))
    qkv = _qkv(seed, B, E, S, lines, axis, kind)
    _check(_attention(L, qkv, E, axis), A.attention(qkv.double(), E, axis), A.attention(qkv, E, axis))


# S = 1 ... 80 are one image at either width: S = 1, the four-key groups with tails of 3 and 1, whole waves +- 1.
# S = 1027 is chunked at either width, with two query rounds (the second three queries wide): 1024 + 3 keys at E = 32 (a
# last chunk of the tail loop only), 512 + 512 + 3 at E = 64
@pytest.mark.parametrize("kind", ["n01", "sharp"])
@pytest.mark.parametrize("S", [1, 3, 63, 65, 80, 1027])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("E", [32, 64])
def test_attention(L, E, axis, S, kind):
    _attn_case(L, 300 + S, 2, E, S, 2, axis, kind)


# either side of the threshold between the two paths: the largest single image (512 keys at E = 64; 1024 at E = 32, which
# is also a full workgroup of queries) and one key more (a second chunk of one tail key; at E = 32 a second query round
# one query wide)
@pytest.mark.parametrize("kind", ["n01", "sharp"])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("E,S", [(64, 512), (64, 513), (32, 1024), (32, 1025)])
def test_attention_image_boundary(L, E, S, axis, kind):
    _attn_case(L, 350 + S, 1, E, S, 2, axis, kind)


# several whole chunks: (64, 1030) is 512 + 512 + 6 keys - a last chunk of one four-key group and two tail keys - in two
# query rounds; (32, 2051) is 1024 + 1024 + 3 - a last chunk of the tail loop only - in three rounds
@pytest.mark.parametrize("kind", ["n01", "sharp"])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("E,S,lines", [(64, 1030, 2), (32, 2051, 1)])
def test_attention_key_chunks(L, E, S, lines, axis, kind):
    _attn_case(L, 400 + S, 1, E, S, lines, axis, kind)


# uniform weights, the output is the mean of v: one image (32, 65) and three chunks (64, 1030)
@pytest.mark.parametrize("E,S,axis", [(32, 65, 0), (64, 1030, 1)])
def test_attention_all_keys_equal(L, E, S, axis):
    _attn_case(L, 500 + S, 1, E, S, 2, axis, "flat")


# ------------------------------------------------------------------ bigru
FORMS = {"h64_fused": (64, True, 0), "h64_unfused": (64, False, 0), "h64_split": (64, True, 1), "h128_unfused": (128, False, 0)}


def _gru_weights(seed, H):
    """nn.GRU's initialisation: U(-1/sqrt(H), 1/sqrt(H)); input size H/2 (d_model)."""
    g = _gen(seed)
    k = 1.0 / math.sqrt(H)

    def u(*shape):
        return (torch.rand(*shape, generator=g, dtype=torch.float32) * 2 - 1) * k

    return u(2, 3 * H, H // 2), u(2, 3 * H, H), u(2, 3 * H), u(2, 3 * H)


def _gru_launch(L, form, x, gx, W_ih, W_hh, b_ih, b_hh, axis):
    """One launch of the form, weights packed as the network plan packs them (nets.py, _aia_layer)."""
    P = pkg("packing")
    H, fused, split = FORMS[form]
    B, _, T, F_ = x.shape
    keep = []

    def up(a, dtype=np.float32):
        keep.append(torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV))
        return keep[-1].data_ptr()

    def tiles(W, kin):          # [2 dirs][3H/32 gate tiles][kin/16 K blocks][3 planes][64 lanes][8] bf16
        return np.stack([np.stack([P.pack_s3_gather(W[dr, 32 * m:32 * m + 32].numpy().T, 1, kin)
                                   for m in range(3 * H // 32)], 0) for dr in range(2)], 0).view(np.int16)

    d = L.GruDesc()
    y = torch.full((B, 2 * H, T, F_), SENTINEL, device=DEV)
    d.y, d.B, d.T, d.F, d.H, d.axis, d.split = y.data_ptr(), B, T, F_, H, axis, split
    d.bhh = up(b_hh.numpy())
    if split:
        d.whh, d.wih = up(tiles(W_hh, H), np.int16), up(tiles(W_ih, H // 2), np.int16)
    else:
        d.whh = up(np.stack([P.pack_a(W_hh[dr].numpy().T) for dr in range(2)], 0))
        if fused:
            d.wih = up(np.stack([P.pack_a(W_ih[dr].numpy().T) for dr in range(2)], 0))
    if fused:
        d.x, d.bih = up(x.numpy()), up(b_ih.numpy())
    else:
        d.gx = up(gx.numpy())
    L.launch(d)
    torch.cuda.synchronize()
    return y


def _gru_case(L, form, axis, B, T, F_, scale, seed):
    H = FORMS[form][0]
    W_ih, W_hh, b_ih, b_hh = _gru_weights(seed, H)
    x = _randn(_gen(seed + 1), B, H // 2, T, F_) * scale
    # the unfused forms read the projection gx = W_ih x + b_ih of both directions: computed once in double and rounded
    # to the fp32 tensor the kernel is handed; both references start from that same tensor
    gx = torch.cat([torch.einsum("gi,bitf->bgtf", W_ih[dr].double(), x.double()) + b_ih[dr].double().view(1, -1, 1, 1)
                    for dr in range(2)], dim=1).float()
    got = _gru_launch(L, form, x, gx, W_ih, W_hh, b_ih, b_hh, axis)
    if FORMS[form][1]:
        ref64 = A.bigru(*_d(x, W_ih, W_hh, b_ih, b_hh), axis)
        ref32 = A.bigru(x, W_ih, W_hh, b_ih, b_hh, axis)
    else:
        ref64 = A.bigru(None, None, W_hh.double(), None, b_hh.double(), axis, gx=gx.double())
        ref32 = A.bigru(None, None, W_hh, None, b_hh, axis, gx=gx)
    _check(got, ref64, ref32)


# (axis, B, T, F): 33 lines of 7 steps (one full group of 32 and one line); 5 lines of 80 steps along the bins;
# S = 1; 3 lines of 401 steps (error growth over the workload's own length)
@pytest.mark.parametrize("axis,B,T,F_", [(1, 3, 7, 11), (0, 1, 5, 80), (1, 2, 1, 40), (1, 1, 401, 3)])
@pytest.mark.parametrize("form", list(FORMS))
def test_bigru(L, form, axis, B, T, F_):
    _gru_case(L, form, axis, B, T, F_, 1.0, 600 + T)


@pytest.mark.parametrize("form", list(FORMS))
def test_bigru_saturated_gates(L, form):
    """Inputs scaled by 8: sigmoid and tanh of the gates at either end of their range."""
    _gru_case(L, form, 1, 3, 7, 11, 8.0, 650)


def test_bigru_refusals(L):
    # every pointer aims at one zeroed buffer as large as the largest operand any form reads (W_hh of both directions at
    # H = 128), so a descriptor that slipped past its check would stay inside it and fail the assertions below
    buf = torch.zeros(2 * 3 * 128 * 128, device=DEV)

    def desc(H, fused, split):
        d = L.GruDesc()
        d.gx = d.whh = d.bhh = d.y = buf.data_ptr()
        d.B, d.T, d.F, d.H, d.axis, d.split = 1, 1, 1, H, 1, split
        if fused:
            d.x = d.wih = d.bih = buf.data_ptr()
        return d

    with pytest.raises(L.PdseError, match="hidden size 64 or 128"):
        L.launch(desc(96, False, 0))
    with pytest.raises(L.PdseError, match="fused input projection needs H == 64"):
        L.launch(desc(128, True, 0))
    with pytest.raises(L.PdseError, match="split is 0 or 1"):
        L.launch(desc(64, True, 2))
    torch.cuda.synchronize()
    assert not buf.cpu().any(), "a refused descriptor launched"


# ------------------------------------------------------------------ gn_combine
GN_PARTS = 64           # csrc/aia.hip; include/pdse.h: stats is [B][64][4]


@pytest.mark.parametrize("plane", [1, 37, 960])
@pytest.mark.parametrize("C", [32, 64])
def test_gn_combine(L, C, plane):
    """Every item draws another (mean, std) for row and for col, so statistics mixed between items - or between row and
    col - show; each item is held to the rule on its own, with its own e32."""
    B = 3
    g = _gen(700 + C + plane)
    row_d, col_d = ["n01", "m8", "m64"], ["m64", "n01", "m8"]
    base = _randn(g, B, C, plane)
    row = torch.stack([_randn(g, C, plane) * DISTS[k][1] + DISTS[k][0] for k in row_d])
    col = torch.stack([_randn(g, C, plane) * DISTS[k][1] + DISTS[k][0] for k in col_d])
    g_row, b_row, g_col, b_col = (1 + 0.3 * _randn(g, C), 0.2 * _randn(g, C), 0.8 + 0.3 * _randn(g, C), 0.2 * _randn(g, C))
    k1, k2 = 0.7, -1.3
    dev = [_dev(t) for t in (base, row, col, g_row, b_row, g_col, b_col)]
    stats = torch.zeros(B, GN_PARTS, 4, device=DEV)
    out = torch.full((B, C, plane), SENTINEL, device=DEV)
    d = L.GncombDesc()
    d.base, d.row, d.col, d.g_row, d.b_row, d.g_col, d.b_col = (t.data_ptr() for t in dev)
    d.stats, d.out, d.plane, d.B, d.C, d.k1, d.k2, d.eps = stats.data_ptr(), out.data_ptr(), plane, B, C, k1, k2, 1e-8
    L.launch(d)
    torch.cuda.synchronize()
    ref64 = A.gn_combine(*_d(base, row, col, g_row, b_row, g_col, b_col), k1, k2, 1e-8)
    ref32 = base + k1 * F.group_norm(row, 1, g_row, b_row, 1e-8) + k2 * F.group_norm(col, 1, g_col, b_col, 1e-8)
    out = out.cpu()
    for b in range(B):
        print("item %d: row %s col %s" % (b, row_d[b], col_d[b]))
        _check(out[b], ref64[b], ref32[b])


# ------------------------------------------------------------------ aham
@pytest.mark.parametrize("C,plane", [(64, 1), (64, 255), (5, 1000)])
def test_aham(L, C, plane):
    """Layer offsets (0, 3, -2, 6) times sum(w) ~ 2 put the four logits several units apart: a softmax peaked on the last
    layer for item 0 and, with that layer's offset at -3, on layer 1 for item 1."""
    B = 2
    g = _gen(800 + C)
    xs = [_randn(g, B, C, plane) + off for off in (0.0, 3.0, -2.0, 6.0)]
    xs[3][1] -= 9.0
    w, bias = (torch.rand(C, generator=g) + 0.5) * 2.0 / C, 0.3
    xd, wd = [_dev(x) for x in xs], _dev(w)
    means = torch.zeros(4, B, C, device=DEV)
    out = torch.full((B, C, plane), SENTINEL, device=DEV)
    d = L.AhamDesc()
    for i in range(4):
        d.x[i] = xd[i].data_ptr()
    d.w, d.means, d.out, d.plane, d.B, d.C, d.bias = wd.data_ptr(), means.data_ptr(), out.data_ptr(), plane, B, C, bias
    L.launch(d)
    torch.cuda.synchronize()
    _check(out, A.aham(_d(*xs), w.double(), bias), A.aham(xs, w, bias))


# ------------------------------------------------------------------ crm
@pytest.mark.parametrize("plane", [1, 257])
@pytest.mark.parametrize("mode", [0, 1])
def test_crm(L, mode, plane):
    """o ~ 20 N(0,1): both sigmoids and the tanh saturate at either end.  Where re = im = 0 exactly the phase is
    atan2(0, 0) = 0 and the magnitude 0: the output there is ri, bit for bit."""
    B = 2
    g = _gen(900 + plane)
    x, ri, o = _randn(g, B, 2, plane), _randn(g, B, 2, plane), 20 * _randn(g, B, plane)
    zeros = [(0, 0)] + ([(1, 100), (1, 256)] if plane > 1 else [])
    for b, q in zeros:
        x[b, :, q] = 0.0
    a1, b1, a2, b2, a3, b3 = 1.3, -0.2, 0.8, 0.1, 2.5, -0.4
    xd, od, rd = _dev(x), _dev(o), _dev(ri)
    out = torch.full((B, plane) if mode == 0 else (B, 2, plane), SENTINEL, device=DEV)
    d = L.CrmDesc()
    d.x, d.out, d.plane, d.B, d.mode = xd.data_ptr(), out.data_ptr(), plane, B, mode
    if mode == 1:
        d.o, d.ri = od.data_ptr(), rd.data_ptr()
        d.a1, d.b1, d.a2, d.b2, d.a3, d.b3 = a1, b1, a2, b2, a3, b3
    L.launch(d)
    torch.cuda.synchronize()
    if mode == 0:
        _check(out, A.crm(0, x.double()), A.crm(0, x))
        for b, q in zeros:
            assert float(out[b, q]) == 0.0
        return
    _check(out, A.crm(1, *_d(x, o, ri), a1, b1, a2, b2, a3, b3), A.crm(1, x, o, ri, a1, b1, a2, b2, a3, b3))
    for b, q in zeros:
        assert torch.equal(out[b, :, q].cpu(), ri[b, :, q])
