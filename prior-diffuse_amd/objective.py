"""Host side of the denoising-objective epoch (``ComplexDDPMTrainer.objective``; reference: ``train_step``,
trainer/complex_ddpm_trainer.py:633-760): which loss the config names, and the aggregation of per-batch figures into the
reference's three logged values and a curve over the diffusion steps.  Pure Python on names and numbers, beside
``validation.aggregate``: nothing here touches a device or reads a waveform."""
import numpy as np

# config.train.loss (the name the reference hands to eval(), :668, :738) -> index into ops.spec_losses' three losses
LOSS_NAMES = {"com_mse_loss": 0, "mag_mse_loss": 1, "com_mag_mse_loss": 2}
DEFAULT_LOSS = "com_mag_mse_loss"     # conf/gcrn.yml, conf/dbaiat.yml


def loss_name(config):
    """``config.train.loss``, ``com_mag_mse_loss`` where the config has none; a name outside ``LOSS_NAMES``: ValueError."""
    name = getattr(getattr(config, "train", None), "loss", None) or DEFAULT_LOSS
    if name not in LOSS_NAMES:
        raise ValueError("config.train.loss %r: the losses built are %s" % (name, ", ".join(sorted(LOSS_NAMES))))
    return name


def _numerators(per_utt, k):
    """Per-utterance numerators over the common denominator 2 F frames, from ``spec_losses``' (com, mag) pairs [B][2]:
    com_mse = com / (2 F n); mag_mse = mag / (F n) = 2 mag / (2 F n); com_mag_mse = (com / 2 + mag) / (2 F n)."""
    per_utt = np.asarray(per_utt, dtype=np.float64).reshape(-1, 2)
    return (per_utt[:, 0], 2.0 * per_utt[:, 1], 0.5 * per_utt[:, 0] + per_utt[:, 1])[k]


def aggregate(batches, names, steps, loss=DEFAULT_LOSS, sigma=False, lam=1.0, joint=False, F=161):
    """The dictionary ``objective`` returns, from host numbers.  batches: one dict per (batch, draw) evaluation, in the order they
    ran, with ``names`` (indices into ``names``), ``frames`` [B], ``t`` [B], ``dis`` {"loss" [3], "per_utt" [B][2]} - the prior
    against the label, ``ops.spec_losses``' fields - and ``ddpm``: the same fields for the eps-net's prediction against its
    target, or with ``sigma`` {"loss" [1], "per_utt" [B]}, ``ops.sigma_loss``' fields.  steps: len(noise_schedule).

    ``ddpm_loss``: the mean of the evaluations' losses - what the reference's per-step ``ddpm_loss`` figure averages to - of the
    --sigma loss with ``sigma``, else of the loss ``loss`` names (``LOSS_NAMES``; any other name: ValueError); ``dis_loss``: the
    same loss name on ``dis``; ``loss_sum`` = lam * ddpm_loss + dis_loss, where dis_loss counts only with ``joint``
    (:666-672: without --joint the reference's loss_dis is 0) and is reported either way.  ``ddpm_loss_per_frame`` /
    ``dis_loss_per_frame``: summed numerators over summed denominators 2 F frames, which do not depend on how the files fell
    into batches.  ``by_step``: for every n in 0 .. steps - 1 the (utterance, draw) evaluations at t = n: ``count``, the summed
    numerator ``num``, the summed ``frames`` and ``per_frame`` = num / (2 F frames) - None where the step was never drawn.
    ``files``: per file its name, frames and per draw ``t`` and ``num``."""
    if loss not in LOSS_NAMES:
        raise ValueError("loss %r: the losses built are %s" % (loss, ", ".join(sorted(LOSS_NAMES))))
    if not batches:
        raise ValueError("objective epoch without a batch (no pairs, or drop_last dropped the only one)")
    k = LOSS_NAMES[loss]
    ddpm, dis, num_sum, dis_sum, frame_sum = [], [], 0.0, 0.0, 0
    by_step = [{"t": n, "count": 0, "num": 0.0, "frames": 0, "per_frame": None} for n in range(int(steps))]
    files = {}
    for b in batches:
        ddpm.append(float(np.asarray(b["ddpm"]["loss"]).reshape(-1)[0 if sigma else k]))
        dis.append(float(np.asarray(b["dis"]["loss"]).reshape(-1)[k]))
        num = np.asarray(b["ddpm"]["per_utt"], dtype=np.float64).reshape(-1) if sigma else _numerators(b["ddpm"]["per_utt"], k)
        dnum = _numerators(b["dis"]["per_utt"], k)
        for j, i in enumerate(b["names"]):
            t, fr = int(b["t"][j]), int(b["frames"][j])
            if not 0 <= t < len(by_step):
                raise ValueError("diffusion step %d outside the %d-entry noise schedule" % (t, len(by_step)))
            row = by_step[t]
            row["count"], row["num"], row["frames"] = row["count"] + 1, row["num"] + float(num[j]), row["frames"] + fr
            files.setdefault(i, {"name": names[i], "frames": fr, "draws": []})["draws"].append({"t": t, "num": float(num[j])})
            num_sum, dis_sum, frame_sum = num_sum + float(num[j]), dis_sum + float(dnum[j]), frame_sum + fr
    for row in by_step:
        if row["frames"]:
            row["per_frame"] = row["num"] / (2.0 * F * row["frames"])
    res = {"loss": "com_mse_sigma_loss" if sigma else loss, "dis_loss_name": loss, "lam": float(lam), "joint": bool(joint)}
    res["ddpm_loss"], res["dis_loss"] = float(np.mean(ddpm)), float(np.mean(dis))
    res["loss_sum"] = float(lam) * res["ddpm_loss"] + (res["dis_loss"] if joint else 0.0)
    res["ddpm_loss_per_frame"] = num_sum / (2.0 * F * frame_sum)
    res["dis_loss_per_frame"] = dis_sum / (2.0 * F * frame_sum)
    res["by_step"] = by_step
    res["files"] = [files[i] for i in sorted(files)]
    res["batches"] = len(batches)
    return res


def log_line(res):
    """The one line of an epoch: the reference's three wandb keys (:743-749), the per-frame figure and how many steps were met."""
    met = [row for row in res["by_step"] if row["count"]]
    line = "dis_loss %.6g ddpm_loss %.6g loss_sum %.6g ddpm_loss_per_frame %.6g" % (res["dis_loss"], res["ddpm_loss"], res["loss_sum"],
                                                                                   res["ddpm_loss_per_frame"])
    return line + " steps_met %d/%d evaluations %d (%s)" % (len(met), len(res["by_step"]), sum(r["count"] for r in met), res["loss"])
