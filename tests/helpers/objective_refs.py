"""numpy restatement of the denoising objective's elementwise arithmetic (trainer/complex_ddpm_trainer.py:699-738, utils/loss.py)
in fp32, every operation rounded on its own as torch's tensor operations round them, and the float64 sums of the fp32 loss terms
the kernels of csrc/objective.hip and csrc/valid.hip add.  Also the seeded inputs of tests/golden/objective_step.npz, which the
tool that writes the fixture and the tests that read it both take from here."""
import numpy as np

MODES = ("pirorgrad", "deltamu", "plain")
B, T, F = 3, 5, 161
FRAMES = (5, 3, 2)
STEPS = (0, 49, 17)
SEED = 1100
F32 = np.float32


def seeded(shape, seed):
    import torch

    g = torch.Generator().manual_seed(int(seed))
    return torch.randn(*shape, generator=g, dtype=torch.float32).numpy()


def raw_inputs():
    """(label, init, noise, predicted) of the fixture BEFORE the division by 11, fp32 [3,2,5,161].  Utterance 1 (3 of 5 frames)
    holds the maximum of |init| of its re plane in a padding frame - the reference takes the maximum over the whole padded plane.
    Utterance 2's padding frames are zeros in all four, as the collate of a silent tail leaves them (and to keep the fixture
    small); utterance 1's are as full as its own frames."""
    shape = (B, 2, T, F)
    label = F32(4.0) * seeded(shape, SEED)
    init = label + F32(2.0) * seeded(shape, SEED + 1)
    noise = seeded(shape, SEED + 2)
    predicted = noise + F32(0.4) * seeded(shape, SEED + 3)
    for x in (label, init, noise, predicted):
        x[2, :, FRAMES[2]:] = 0
    init[1, 0, 4, 7] = F32(99.0)
    return label, init, noise, predicted


def inputs():
    """(label, init, noise, predicted) as the kernels take them: label and init divided by 11 in fp32 (:699-700)."""
    label, init, noise, predicted = raw_inputs()
    return label / F32(11), init / F32(11), noise, predicted


def tables(noise_schedule=None):
    """(a, s): sqrt(alpha_bar) and sqrt(1 - alpha_bar) in fp32 from the float32 cast of the float64 cumprod (:42-44, :710, :726)."""
    beta = np.linspace(1e-4, 0.05, 50) if noise_schedule is None else np.array(noise_schedule, dtype=np.float64)
    level = np.cumprod(1 - beta).astype(F32)
    return np.sqrt(level), np.sqrt(F32(1.0) - level)


def mask_of(init):
    """(mask, maxbuf [B*2]): |init| / max / 2 + 0.5 per (b, channel) plane, the maximum over the whole plane (:713-716)."""
    tmp = np.abs(init.astype(F32)).reshape(init.shape[0], init.shape[1], -1)
    mx = tmp.max(axis=2, keepdims=True)
    tmp = tmp / mx
    tmp = tmp / F32(2) + F32(0.5)
    return tmp.reshape(init.shape).astype(F32), mx.reshape(-1).astype(F32)


def noising(label, init, t, noise, mode, sigma, noise_schedule=None):
    """-> (noisy, target, maxbuf) of :709-733; label, init already divided by 11."""
    label, init, noise = label.astype(F32), init.astype(F32), noise.astype(F32)
    a, s = tables(noise_schedule)
    a, s = a[np.asarray(t)][:, None, None, None], s[np.asarray(t)][:, None, None, None]
    maxbuf = np.zeros(2 * label.shape[0], dtype=F32)
    target = noise.copy()
    if sigma:
        mask, maxbuf = mask_of(init)
        target = noise * np.sqrt(mask)
    if mode == "pirorgrad":
        noisy = a * (label - init) + s * target
    elif mode == "deltamu":
        noisy = a * label + s * (target + init)
    else:
        noisy = a * label + s * target
    assert noisy.dtype == F32 and target.dtype == F32
    return noisy, target, maxbuf


def sigma_loss(predicted, target, init, maxbuf, frames):
    """com_mse_sigma_loss (utils/loss.py:46-56): -> (per_utt [B] float64 sums of the fp32 terms (d / mask) d over the live
    frames, the loss in double).  The mask is recomputed from init and maxbuf as pdse_sigma_loss recomputes it."""
    p, tg, init = predicted.astype(F32), target.astype(F32), init.astype(F32)
    nb = p.shape[0]
    mx = np.asarray(maxbuf, dtype=F32).reshape(nb, 2, 1, 1)
    mask = np.abs(init) / mx
    mask = mask * F32(0.5) + F32(0.5)
    per = np.zeros(nb)
    for b, fr in enumerate(frames):
        d = p[b, :, :fr] - tg[b, :, :fr]
        term = (d / mask[b, :, :fr]) * d
        assert term.dtype == F32
        per[b] = term.astype(np.float64).sum()
    return per, per.sum() / (2.0 * p.shape[-1] * float(sum(frames)))


def spec_losses(esti, label, frames):
    """com_mse, mag_mse and com_mag_mse (utils/loss.py:34-44, :10-19, :59-71): -> (per_utt [B][2] float64 sums of the fp32 terms
    pdse_spec_losses adds, (com_mse, mag_mse, com_mag_mse) in double)."""
    e, l = esti.astype(F32), label.astype(F32)
    per = np.zeros((e.shape[0], 2))
    for b, fr in enumerate(frames):
        d = e[b, :, :fr] - l[b, :, :fr]
        per[b, 0] = (d * d).astype(np.float64).sum()
        me = np.sqrt(e[b, 0, :fr] * e[b, 0, :fr] + e[b, 1, :fr] * e[b, 1, :fr])
        ml = np.sqrt(l[b, 0, :fr] * l[b, 0, :fr] + l[b, 1, :fr] * l[b, 1, :fr])
        dm = me - ml
        per[b, 1] = (dm * dm).astype(np.float64).sum()
    n = float(sum(frames)) * e.shape[-1]
    com, mag = per[:, 0].sum() / (2 * n), per[:, 1].sum() / n
    return per, (com, mag, 0.5 * (com + mag))


def case_key(mode, sigma):
    return "%s_%s" % (mode, "sigma" if sigma else "plain")
