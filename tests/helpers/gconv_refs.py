"""A plain torch statement of the gather-GEMM convolution of include/pdse.h (pdse_gconv_desc, epilogues LINEAR and GLU):
the reference of tests/test_gpu_gconv_ops.py.  It takes plain tensors and k-major weight matrices - no descriptor, no
packed weights - and imports nothing of the package under test nor of tests/emu.py; tests/test_gconv_refs_host.py holds
it to torch's own convolutions in double.

    acc[co](b, t, j) = sum_tap sum_ci Wk[tap * Cin + ci][co] * IN(b, ci, t + dt[tap], j * sf_in + df[tap])

  1. gather: IN is zero outside [0,Tin) x [0,Fin); with ``padrow`` [B, Cin], frame -1 reads padrow[b][ci] (bins still
     have to be in range; frames <= -2 stay zero).  The per-source activation applies to the values of the tensor;
  2. the load transform prelu(v, slope) * scale[ci] + shift[ci] applies to in-bounds values only (neither to the zero
     padding nor to the pad row); xf mode 1: one set for both accumulators, mode 2: set 0 -> acc0, set 1 -> acc1;
  3. tap table and sf_in as above; ``cin1``: one input channel, k enumerates the taps;
  4. + bias ([Cout] shared, or [B, Cout] per item);
  5. GLU: y = (acc0 + bias0) * sigmoid(acc1 + bias1); then y * post_scale + post_shift, the activation, + resid.
"""
import torch

ACT_NONE, ACT_PRELU, ACT_ELU, ACT_SIGMOID = 0, 1, 2, 3      # enum pdse_act
EPI_LINEAR, EPI_GLU = 0, 1                                   # enum pdse_epi


def act(v, kind, slope=0.0):
    if kind == ACT_PRELU:
        return torch.where(v > 0, v, slope * v)
    if kind == ACT_ELU:
        return torch.where(v > 0, v, torch.expm1(torch.clamp(v, max=0)))
    if kind == ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


def bf16_rne(v):
    """Round to the nearest bf16 (ties to even) by way of fp32, the format the kernels hold the value in."""
    return v.to(torch.float32).to(torch.bfloat16).to(v.dtype)


def gconv(in0, in1=None, *, taps, Wk0, Wk1=None, Tout, Fout, sf_in=1, act0=ACT_NONE, act1=ACT_NONE, padrow=None, xf=None,
          cin1=False, bias0=None, bias1=None, epi=EPI_LINEAR, post_scale=None, post_shift=None, act_out=ACT_NONE,
          act_slope=0.0, resid=None, dtype=torch.float64, round_operands=None):
    """in0 [B, C0, Tin, Fin] (in1 [B, C1, Tin, Fin]: channel concatenation behind in0); taps: [(dt, df)];
    Wk0 (Wk1: the gate of GLU) [ntaps * Cin, Cout]; xf: dict(mode, slope0, scale0, shift0[, slope1, scale1, shift1]);
    resid [B, Cout, Tout, Fout].  Everything is evaluated in ``dtype``.  round_operands "bf16": the weights and the
    gathered activations (after the load-side activation) are rounded to bf16 before the contraction, whose products
    are then exact in either dtype.  Returns [B, Cout, Tout, Fout]."""
    assert round_operands in (None, "bf16")
    cv = lambda x: None if x is None else torch.as_tensor(x).to(dtype)      # noqa: E731
    srcs = [(cv(in0), act0)] + ([(cv(in1), act1)] if in1 is not None else [])
    B, _, Tin, Fin = srcs[0][0].shape
    Cin = sum(s.shape[1] for s, _ in srcs)
    W = [cv(Wk0)] + ([cv(Wk1)] if epi == EPI_GLU else [])
    if round_operands:
        W = [bf16_rne(w) for w in W]
    ntaps, Cout = len(taps), W[0].shape[1]
    assert W[0].shape[0] == ntaps * Cin and (not cin1 or Cin == 1)
    padrow = cv(padrow)
    x = torch.cat([act(s, a) for s, a in srcs], dim=1)                        # [B, Cin, Tin, Fin]
    tI, jI = torch.arange(Tout).view(-1, 1), torch.arange(Fout).view(1, -1)
    acc = [torch.zeros(B, Cout, Tout, Fout, dtype=dtype) for _ in W]
    for k, (dt, df) in enumerate(taps):
        tin, fin = (tI + dt).expand(Tout, Fout), (jI * sf_in + df).expand(Tout, Fout)
        fok = (fin >= 0) & (fin < Fin)
        inb = fok & (tin >= 0) & (tin < Tin)
        v = x[:, :, tin.clamp(0, Tin - 1), fin.clamp(0, Fin - 1)]            # [B, Cin, Tout, Fout]
        v = torch.where(inb, v, torch.zeros((), dtype=dtype))
        if round_operands:
            v = bf16_rne(v)
        vs = [v] * len(W)
        if xf is not None and xf["mode"]:
            vs = []
            for i in range(len(W)):
                s = str(i if xf["mode"] == 2 else 0)
                u = act(v, ACT_PRELU, float(xf["slope" + s]))
                u = u * cv(xf["scale" + s]).view(1, -1, 1, 1) + cv(xf["shift" + s]).view(1, -1, 1, 1)
                vs.append(torch.where(inb, u, v))
        if padrow is not None:
            isp = (fok & (tin == -1)).expand(B, Cin, Tout, Fout)
            vs = [torch.where(isp, padrow[:, :, None, None].expand(B, Cin, Tout, Fout), u) for u in vs]
        for a, w, u in zip(acc, W, vs):
            a += torch.einsum("km,bktf->bmtf", w[k * Cin:(k + 1) * Cin], u)

    def bias(bv):
        return 0 if bv is None else cv(bv).view(-1, Cout, 1, 1)

    y = acc[0] + bias(bias0)
    if epi == EPI_GLU:
        y = y * torch.sigmoid(acc[1] + bias(bias1))
    if post_scale is not None:
        y = y * cv(post_scale).view(1, -1, 1, 1) + cv(post_shift).view(1, -1, 1, 1)
    y = act(y, act_out, float(act_slope))
    if resid is not None:
        y = y + cv(resid)
    return y
