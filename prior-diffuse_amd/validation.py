"""Host side of the validation epoch (``ComplexDDPMTrainer.validate``; reference: trainer/complex_ddpm_trainer.py:399-580):
pairing of the two directories, the batches of an epoch, the frame arithmetic and the aggregation of per-batch figures.  Pure
Python on names and numbers: nothing here touches a device or reads a waveform."""
import glob
import os

import numpy as np

HOP = 160
LOSSES = ("com_mse", "mag_mse", "com_mag_mse")
MEASURES = ("ssnr", "llr", "wss", "fwsnrseg")
STOI_MEASURES = ("stoi", "estoi")


def frame_num(n):
    """Frames of an utterance of n samples: (n - win_size + fft_num) // win_shift + 1 (utils/dataset.py:152, 320 / 320 / 160)."""
    return int(n) // HOP + 1


def trim_len(n):
    """Samples compare_complex keeps of an utterance of n samples: (frame_num - 1) * 160 (utils/metrics.py:562-563)."""
    return (frame_num(n) - 1) * HOP


def pair_names(noisy_dir, clean_dir):
    """The (noisy path, clean path) pairs of an epoch in name order: every ``*.wav`` of ``noisy_dir`` with the file of the same
    name in ``clean_dir`` (VBCvDataset, utils/dataset.py:133-153).  A noisy file without a partner: ValueError naming it."""
    pairs = []
    for path in sorted(glob.glob(os.path.join(noisy_dir, "*.wav"))):
        partner = os.path.join(clean_dir, os.path.basename(path))
        if not os.path.isfile(partner):
            raise ValueError("validation pair: %s has no clean partner %s" % (path, partner))
        pairs.append((path, partner))
    return pairs


def check_lengths(pairs, noisy_lens, clean_lens):
    """Both files of a pair hold the same number of samples (at 16 kHz), else ValueError naming the noisy file."""
    for (path, partner), n, m in zip(pairs, noisy_lens, clean_lens):
        if int(n) != int(m):
            raise ValueError("validation pair: %s holds %d samples, its clean partner %s holds %d" % (path, int(n), partner, int(m)))


def windows(n, batch_size, order="sorted", drop_last=False):
    """The batches of an epoch over n sorted names, as lists of indices.  "sorted": windows of ``batch_size`` consecutive names -
    every file once, in a reproducible order.  "shuffled": the same windows of one ``torch.randperm(n)`` drawn from the global
    generator (the reference's DataLoader shuffles).  drop_last: without the last, partial batch (the reference drops it)."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1, got %d" % batch_size)
    if order not in ("sorted", "shuffled"):
        raise ValueError("order must be 'sorted' or 'shuffled'")
    if order == "shuffled":
        import torch

        idx = torch.randperm(n).tolist()
    else:
        idx = list(range(n))
    out = [idx[i:i + batch_size] for i in range(0, n, batch_size)]
    if drop_last and out and len(out[-1]) < batch_size:
        out.pop()
    return out


def _section(batches, F, stoi):
    """batches: [{"loss": (com, mag, com_mag), "per_utt": [B][2], "frames": [B], <measure>: [B]}] of one scored signal."""
    res = {}
    com = sum(float(u[0]) for b in batches for u in b["per_utt"])
    mag = sum(float(u[1]) for b in batches for u in b["per_utt"])
    frames = sum(int(f) for b in batches for f in b["frames"])
    per_frame = (com / (2.0 * F * frames), mag / (1.0 * F * frames))
    per_frame += (0.5 * (per_frame[0] + per_frame[1]),)
    for k, name in enumerate(LOSSES):
        key = "loss" if name == "com_mse" else name            # "loss": the reference's cv_loss / test_com_mse_loss
        res[key] = float(np.mean([float(b["loss"][k]) for b in batches]))
        res[key + "_per_frame"] = float(per_frame[k])
    for m in MEASURES + (STOI_MEASURES if stoi else ()):
        res["mean_" + m] = float(np.mean([float(np.mean(np.asarray(b[m], dtype=np.float64))) for b in batches]))   # means of batch means
    return res


def aggregate(batches, names, F=161, prior=True, stoi=False):
    """The dictionary ``validate`` returns, from per-batch host numbers.  batches: one dict per batch with ``names`` (indices
    into ``names``), ``frames`` and the scored signals "x" and, with ``prior``, "init" (``_section``'s fields).
    ``loss`` is the mean of the batches' com_mse - np.mean(all_loss_list), the figure that selects best_checkpoint.pth (:581) -
    and ``loss_per_frame`` the summed numerators over the summed denominators, which does not depend on how the files fell
    into batches; the same pair for ``mag_mse`` and ``com_mag_mse``; ``mean_<measure>`` are means of batch means, like the
    reference's np.mean over compare_complex's per-batch means."""
    if not batches:
        raise ValueError("validation epoch without a batch (no pairs, or drop_last dropped the only one)")
    sections = ("x", "init") if prior else ("x",)
    sec = {s: _section([dict(b[s], frames=b["frames"]) for b in batches], F, stoi) for s in sections}
    res = dict(sec["x"])
    if prior:
        res["init"] = sec["init"]
    files = []
    for b in batches:
        for j, i in enumerate(b["names"]):
            row = {"name": names[i], "frames": int(b["frames"][j])}
            for s in sections:
                d = row if s == "x" else row.setdefault("init", {})
                d["com_num"], d["mag_num"] = float(b[s]["per_utt"][j][0]), float(b[s]["per_utt"][j][1])
                for m in MEASURES + (STOI_MEASURES if stoi else ()):
                    d[m] = float(b[s][m][j])
            files.append(row)
    res["files"] = files
    res["batches"] = len(batches)
    return res


def log_line(res):
    """The one line of an epoch: the reference's wandb keys (:561-570) less PESQ and the composites, the prior's behind them."""
    def part(d, suffix):
        keys = [("test_com_mse_loss", "loss"), ("test_mag_mse_loss", "mag_mse"), ("test_com_mag_mse_loss", "com_mag_mse")]
        keys += [("test_mean_" + m, "mean_" + m) for m in MEASURES + STOI_MEASURES if "mean_" + m in d]
        return " ".join("%s%s %.6g" % (k, suffix, d[v]) for k, v in keys)

    line = part(res, "")
    if "init" in res:
        line += " " + part(res["init"], "_init")
    return line
