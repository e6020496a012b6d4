"""A plain torch statement of one residual block of the eps-net's temporal convolution modules, fused the way the
TCM kernels fuse it (include/pdse.h: pdse_tcm_desc, pdse_tcm2_desc) - with the NEXT block's 1x1 input convolution:

    h   = W1 x + b1                                                          (1x1, 256 -> 64)
    g   = (Wm * BN_m(PReLU_m(h)) + bm) . sigmoid(Wk * BN_k(PReLU_k(h)) + bk)   (k = 5, dilation d, zero padding 2 d)
    x'  = W2 BN_2(PReLU_2(g)) + b2 + x                                       (1x1, 64 -> 256)
    h'  = W1next x' + b1next

Natural parameters only (a dict per block, see KEYS): convolution weights in torch's own layout, eval-mode BatchNorm as
(scale, shift), PReLU slopes as numbers.  No packing, no fragment order.  The zero padding of the dilated convolutions
is applied AFTER BatchNorm (the padded tensor is the transformed one), which is why the kernels exchange BN(PReLU(h)).

``frames``: utterance b computed as if it were alone with frames[b] frames (clamped to 0..T): the transformed h is
zero from frames[b] on.  Values at t >= frames[b] are returned as they come out (callers compare own frames only),
except the next block's transforms, which are zero there.

``rnd``: round to bf16 (nearest even) at exactly the points at which the one-plane form (np = 1) of csrc/tcm2.hip rounds:
the transformed h of either block, the gate output in front of conv2, x' in front of the chained conv1 (the stored x'
stays unrounded) and every weight; biases, BatchNorm and slopes stay as they are.

Test infrastructure: held to torch.nn's Conv1d / PReLU / BatchNorm1d by tests/test_tcm_refs_host.py."""
import torch
import torch.nn.functional as F

KEYS = ("W1", "b1",                                    # conv1: [64, 256], [64]
        "a_main", "s_main", "t_main", "Wm", "bm",      # main branch: slope, BN scale / shift [64], [64, 64, 5], [64]
        "a_mask", "s_mask", "t_mask", "Wk", "bk",      # mask branch
        "a2", "s2", "t2", "W2", "b2")                  # conv2: slope, BN scale / shift [64], [256, 64], [256]


def bf16(v):
    """What v_cvt_pk_bf16_f32 keeps of the value the kernel holds there: the fp32 value, rounded to 8 significand bits,
    ties to even; returned in the tensor's own dtype."""
    m, e = torch.frexp(v.to(torch.float32).to(torch.float64))
    return (torch.round(m * 256.0) * torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 8).to(torch.float64))).to(v.dtype)


def _t(v, dtype):
    return torch.as_tensor(v).to(dtype)


def _col(v, dtype):
    return _t(v, dtype).view(1, -1, 1)


def _prelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def conv1(x, p, dtype=torch.float64, rnd=False):
    """h = W1 x + b1; rnd: x and W1 as bf16."""
    W, x = _t(p["W1"], dtype), x.to(dtype)
    if rnd:
        W, x = bf16(W), bf16(x)
    return torch.einsum("ok,bkt->bot", W, x) + _col(p["b1"], dtype)


def transforms(h, p, dtype=torch.float64, frames=None, rnd=False):
    """(BN_m(PReLU_m(h)), BN_k(PReLU_k(h))): what the dilated convolutions pad and read."""
    h = h.to(dtype)
    out = []
    for br in ("main", "mask"):
        v = _prelu(h, float(p["a_" + br])) * _col(p["s_" + br], dtype) + _col(p["t_" + br], dtype)
        if rnd:
            v = bf16(v)
        out.append(_own(v, frames))
    return tuple(out)


def clamp_frames(frames, T):
    return None if frames is None else [min(max(int(f), 0), T) for f in frames]


def _own(v, frames):
    if frames is None:
        return v
    v = v.clone()
    for b, f in enumerate(clamp_frames(frames, v.shape[-1])):
        v[b, :, f:] = 0
    return v


def gate(vm, vk, p, dil, dtype=torch.float64, frames=None, rnd=False):
    """BN_2(PReLU_2(main . sigmoid(mask))) from the transformed h of both branches."""
    vm, vk = _own(vm.to(dtype), frames), _own(vk.to(dtype), frames)
    Wm, Wk = _t(p["Wm"], dtype), _t(p["Wk"], dtype)
    if rnd:
        Wm, Wk = bf16(Wm), bf16(Wk)
    main = F.conv1d(vm, Wm, _t(p["bm"], dtype), dilation=dil, padding=2 * dil)
    mask = F.conv1d(vk, Wk, _t(p["bk"], dtype), dilation=dil, padding=2 * dil)
    g = _prelu(main * torch.sigmoid(mask), float(p["a2"])) * _col(p["s2"], dtype) + _col(p["t2"], dtype)
    return bf16(g) if rnd else g


def conv2(g, x, p, dtype=torch.float64, rnd=False):
    W = _t(p["W2"], dtype)
    if rnd:
        W = bf16(W)
    return torch.einsum("ok,bkt->bot", W, g.to(dtype)) + _col(p["b2"], dtype) + x.to(dtype)


def block(x, p, dil, p_next=None, dtype=torch.float64, frames=None, rnd=False, h=None, v=None):
    """One block.  The kernels start from h (csrc/tcm.hip) or from its two transforms (csrc/tcm2.hip): ``h`` / ``v``
    replace the first line / the first two by the given tensors.  Returns a dict: x_out; with p_next also h_out and
    (vm_next, vk_next), the next block's transforms of h_out (rnd: rounded; frames: zero behind the utterance)."""
    if v is None:
        v = transforms(conv1(x, p, dtype, rnd) if h is None else h, p, dtype, frames, rnd)
    out = dict(x_out=conv2(gate(v[0], v[1], p, dil, dtype, frames, rnd), x, p, dtype, rnd))
    if p_next is not None:
        out.update(head(out["x_out"], p_next, dtype, frames, rnd))
    return out


def head(x, p_next, dtype=torch.float64, frames=None, rnd=False):
    """The chained part alone (mode 1 of csrc/tcm2.hip): h_out = conv1_next(x) and the next block's transforms of it."""
    h = conv1(x, p_next, dtype, rnd)
    vm, vk = transforms(h, p_next, dtype, frames, rnd)
    return dict(h_out=h, vm_next=vm, vk_next=vk)
