"""The float64 references of tests/test_gpu_aia_ops.py (tests/helpers/aia_refs.py) against torch's own modules in
double, so that a layout mistake in a reference cannot pass as a kernel result.  Both sides are float64 evaluations of
the same formula: they agree to 1e-12."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import aia_refs as A

TOL = 1e-12


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_rowln_prelu_is_layer_norm_then_prelu():
    B, C, T, F_ = 2, 3, 5, 65
    x = _rand(B, C, T, F_, seed=1) * 0.25 + 64
    gamma, beta = 1 + 0.3 * _rand(F_, seed=2), 0.2 * _rand(F_, seed=3)
    slope = torch.tensor([-0.5, 0.0, 1.7], dtype=torch.float64)
    want = F.prelu(F.layer_norm(x, (F_,), gamma, beta, 1e-5), slope)
    assert _rel(A.rowln_prelu(x, gamma, beta, slope, 1e-5), want) < TOL


@pytest.mark.parametrize("C", [1, 16, 64])
def test_chln_is_layer_norm_over_channels(C):
    x = _rand(2, C, 37, seed=4) + 8
    gamma, beta = 1 + 0.3 * _rand(C, seed=5), 0.2 * _rand(C, seed=6)
    want = F.layer_norm(x.permute(0, 2, 1), (C,), gamma, beta, 1e-5).permute(0, 2, 1)
    assert _rel(A.chln(x, gamma, beta, 1e-5), want) < TOL


@pytest.mark.parametrize("E", [32, 64])
@pytest.mark.parametrize("axis", [0, 1])
def test_attention_is_multi_head_attention_with_identity_projections(E, axis):
    B, T, F_ = 2, 5, 7
    qkv = _rand(B, 3 * E, T, F_, seed=7 + axis)
    got = A.attention(qkv, E, axis)
    # nn.MultiheadAttention's functional form on sequence-first [S, N, E]; it scales q by head_dim^-0.5 itself, so it
    # is handed q * head_dim^0.5
    hd = E // 4
    q, k, v = (A._lines(t, axis) for t in qkv.split(E, dim=1))
    eye = torch.eye(E, dtype=torch.float64)
    want, _ = F.multi_head_attention_forward(
        q * hd ** 0.5, k, v, E, 4, None, None, None, None, False, 0.0, eye, None, training=False, need_weights=False,
        use_separate_proj_weight=True, q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye)
    S, N, _ = want.shape
    want = (want.reshape(F_, B, T, E).permute(1, 3, 2, 0) if axis == 0 else want.reshape(T, B, F_, E).permute(1, 3, 0, 2))
    assert got.shape == (B, E, T, F_)
    assert _rel(got, want) < TOL


@pytest.mark.parametrize("H,I", [(64, 32), (128, 64)])
@pytest.mark.parametrize("axis", [0, 1])
def test_bigru_is_nn_gru_bidirectional(H, I, axis):
    B, T, F_ = 2, 5, 3
    torch.manual_seed(11)
    gru = torch.nn.GRU(I, H, 1, bidirectional=True).double()
    x = _rand(B, I, T, F_, seed=12 + axis)
    sd = gru.state_dict()
    W_ih = torch.stack([sd["weight_ih_l0"], sd["weight_ih_l0_reverse"]])
    W_hh = torch.stack([sd["weight_hh_l0"], sd["weight_hh_l0_reverse"]])
    b_ih = torch.stack([sd["bias_ih_l0"], sd["bias_ih_l0_reverse"]])
    b_hh = torch.stack([sd["bias_hh_l0"], sd["bias_hh_l0_reverse"]])
    with torch.no_grad():
        y, _ = gru(A._lines(x, axis))                                  # [S, N, 2H] = [fw | bw]
    want = (y.reshape(F_, B, T, 2 * H).permute(1, 3, 2, 0) if axis == 0 else y.reshape(T, B, F_, 2 * H).permute(1, 3, 0, 2))
    got = A.bigru(x, W_ih, W_hh, b_ih, b_hh, axis)
    assert got.shape == (B, 2 * H, T, F_)
    assert _rel(got, want) < TOL
    # the gx form: the projections of both directions as one [B,6H,T,F] tensor
    gx = torch.cat([torch.einsum("gi,bitf->bgtf", W_ih[d], x) + b_ih[d].view(1, -1, 1, 1) for d in range(2)], dim=1)
    assert _rel(A.bigru(None, None, W_hh, None, b_hh, axis, gx=gx), want) < TOL


def test_gn_combine_is_group_norm_of_one_group():
    B, C, plane = 3, 32, 37
    base, row, col = _rand(B, C, plane, seed=20), _rand(B, C, plane, seed=21) * 0.25 + 64, _rand(B, C, plane, seed=22) + 8
    g_row, b_row, g_col, b_col = (_rand(C, seed=23 + i) for i in range(4))
    k1, k2 = 0.7, -1.3
    want = base + k1 * F.group_norm(row, 1, g_row, b_row, 1e-8) + k2 * F.group_norm(col, 1, g_col, b_col, 1e-8)
    assert _rel(A.gn_combine(base, row, col, g_row, b_row, g_col, b_col, k1, k2, 1e-8), want) < TOL


def test_aham_is_the_models_softmax_over_layers():
    """model/dbaiat.py:268-288 restated on [B,C,T,F]: y_i = conv1(avgpool(x_i)); out = x_3 + [x_0..x_3] softmax(y)."""
    B, C, T, F_ = 2, 5, 4, 6
    xs = [_rand(B, C, T, F_, seed=30 + i) + off for i, off in enumerate((0.0, 1.0, -0.5, 2.0))]
    w, bias = _rand(C, seed=35), 0.3
    ys = [F.conv2d(F.adaptive_avg_pool2d(x, 1), w.view(1, C, 1, 1), torch.tensor([bias], dtype=torch.float64)) for x in xs]
    x_merge = torch.stack(xs, dim=-1)                                              # [B,C,T,F,4]
    y_soft = torch.softmax(torch.stack(ys, dim=-2), dim=-2)                        # [B,1,1,4,1]
    want = xs[-1] + torch.matmul(x_merge, y_soft).view(B, C, T, F_)
    got = A.aham([x.reshape(B, C, T * F_) for x in xs], w, bias).view(B, C, T, F_)
    assert _rel(got, want) < TOL


def test_crm_is_the_models_mask_and_phase_recombination():
    """model/dbaiat.py:389, :407-411 and the scalar gate of :579-583 restated with 1x1 convolutions."""
    B, T, F_ = 2, 3, 5
    x, ri, o = _rand(B, 2, T, F_, seed=40), _rand(B, 2, T, F_, seed=41), 4 * _rand(B, 1, T, F_, seed=42)
    x[0, :, 1, 2] = 0.0                                                            # |x| = 0: atan2(0, 0) = 0
    a1, b1, a2, b2, a3, b3 = 1.3, -0.2, 0.8, 0.1, 2.5, -0.4

    def conv(t, a, b):
        return F.conv2d(t, torch.full((1, 1, 1, 1), a, dtype=torch.float64), torch.tensor([b], dtype=torch.float64))

    mask = torch.sigmoid(conv(torch.sigmoid(conv(o, a1, b1)) * torch.tanh(conv(o, a2, b2)), a3, b3)).squeeze(1)
    mag, phase = torch.norm(x, dim=1), torch.atan2(x[:, -1], x[:, 0])
    want = torch.stack((mask * mag * torch.cos(phase) + ri[:, 0], mask * mag * torch.sin(phase) + ri[:, 1]), dim=1)
    flat = lambda t: t.reshape(B, -1, T * F_)                                      # noqa: E731
    got = A.crm(1, flat(x), o.reshape(B, T * F_), flat(ri), a1, b1, a2, b2, a3, b3)
    assert _rel(got, flat(want)) < TOL
    assert torch.equal(got[0, :, 1 * F_ + 2], flat(ri)[0, :, 1 * F_ + 2])
    assert _rel(A.crm(0, flat(x)), mag.reshape(B, T * F_)) < TOL


# ------------------------------------------------------------------ GroupNorm statistics of csrc/aia.hip, emulated
def _emulate_gn(x, pivoted):
    """The summation order of gn_stats_kernel / gn_apply_kernel on one item x (float32, flat), in numpy float32:
    64 parts x 256 threads, element i to part (i / 256) % 64, thread i % 256; per-thread running sums, a 64-lane
    butterfly, four waves added left to right; the apply pass folds the parts in double.  pivoted False is the formula
    this replaces: raw sums, var = E[x^2] - mean^2 on moments rounded to float32."""
    f32 = np.float32
    n = x.size
    pad = np.zeros(-(-n // 16384) * 16384, f32)
    p = x[0] if pivoted else f32(0)
    pad[:n] = x - p
    pad = pad.reshape(-1, 64, 256)                                                 # [trip, part, thread]
    s1 = np.zeros((64, 256), f32)
    s2 = np.zeros((64, 256), f32)
    for t in range(pad.shape[0]):
        s1 = s1 + pad[t]
        s2 = s2 + pad[t] * pad[t]

    def block(s):                                                                  # [64, 256] -> [64]
        s = s.reshape(64, 4, 64)
        for off in (32, 16, 8, 4, 2, 1):
            s = s + s[:, :, np.arange(64) ^ off]
        w = s[:, :, 0]
        return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]

    S1, S2 = block(s1).astype(np.float64).sum(), block(s2).astype(np.float64).sum()
    if pivoted:
        m = S1 / n
        mean, rstd = f32(np.float64(p) + m), f32(1.0 / np.sqrt(max(S2 / n - m * m, 0.0) + 1e-8))
    else:
        mean, ex2 = f32(S1 / n), f32(S2 / n)
        rstd = f32(1) / np.sqrt(max(ex2 - mean * mean, f32(0)) + f32(1e-8), dtype=f32)
    return (x - mean) * rstd


@pytest.mark.parametrize("mean,std", [(0.0, 1.0), (8.0, 1.0), (64.0, 0.25)])
def test_gn_variance_formula_emulated(mean, std):
    """C = 32, plane = 960: the pivoted moments of gn_stats_kernel stay within the operator tests' tolerance rule
    max(4 e32, 2e-6) on all three input distributions; the raw E[x^2] - mean^2 they replace does not at (64, 0.25)."""
    C, plane = 32, 960
    x = (_rand(1, C, plane, seed=50) * std + mean).float()
    exact = F.group_norm(x.double(), 1, eps=1e-8)
    e32 = _rel(F.group_norm(x, 1, eps=1e-8).double(), exact)
    bound = max(4 * e32, 2e-6)
    new = _rel(torch.from_numpy(_emulate_gn(x.numpy().ravel(), True)).double().view(1, C, plane), exact)
    old = _rel(torch.from_numpy(_emulate_gn(x.numpy().ravel(), False)).double().view(1, C, plane), exact)
    print("gn (%g, %g): pivoted %.2e  raw moments %.2e  torch fp32 %.2e  bound %.2e" % (mean, std, new, old, e32, bound))
    assert new <= bound
    if mean == 64.0:
        assert old > 100 * bound
