"""CLI mirror of the reference's ``main.py`` for the ``--generate`` and ``--eval`` paths
(main.py:20-101): same flags, same derived directories, YAML config -> Namespace.

    python -m prior_diffuse_amd.main --retrain --assets A --sigma --joint --generate
    python -m prior_diffuse_amd.main --retrain --assets A --joint --eval --data NOISY --clean CLEAN
    python -m prior_diffuse_amd.main --retrain --assets A --joint --eval --objective --draws 4 --data NOISY --clean CLEAN

``--eval`` runs one validation epoch (``ComplexDDPMTrainer.validate``), logs its line and writes the dictionary to
``<assets>/log/<doc>/eval.json``; with ``--generate`` the generation runs, as the reference tests ``generate`` first (:97).
``--eval --objective`` runs one epoch of the denoising objective instead (``ComplexDDPMTrainer.objective``: the eps-net's loss
on the held-out pairs, by diffusion step) and writes ``<assets>/log/<doc>/objective.json``.
``--members K`` makes either a posterior ensemble: ``--generate`` writes every file from the mean of K reverse trajectories and
``<assets>/log/<doc>/ensemble.json``, ``--eval`` scores the mean and adds the members' losses to ``eval.json``.
"""
import argparse
import logging
import os

import numpy as np
import torch
import yaml

from . import longplan


def dict2namespace(config):  # main.py:9-17
    ns = argparse.Namespace()
    for key, value in config.items():
        setattr(ns, key, dict2namespace(value) if isinstance(value, dict) else value)
    return ns


def parse_args_and_config(argv=None):
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--seed", type=int, default=1234, help="Random seed")
    p.add_argument("--trainer", type=str, default="ComplexDDPMTrainer", help="The trainer to execute")
    p.add_argument("--config", type=str, default="diff.yml", help="Path to the config file")
    p.add_argument("--verbose", type=str, default="info", help="Verbose level: info | debug | warning | critical")
    p.add_argument("--doc", type=str, default="diff", help="A string for documentation purpose")
    p.add_argument("--comment", type=str, default="", help="A string for experiment comment")
    p.add_argument("--assets", type=str, default="assets_dpm", help="Path for saving running related data.")
    for flag in ("generate", "retrain", "joint", "eval", "sigma", "noisy", "draw"):
        p.add_argument("--" + flag, action="store_true")
    p.add_argument("--data", type=str, default="data/noisy_testset_wav", help="directory of noisy wavs")
    p.add_argument("--clean", type=str, default="data/clean_testset_wav",
                   help="(not a flag of the reference) --eval: directory of the clean partners of --data, matched by file name")
    p.add_argument("--bf16", action="store_true",
                   help="(not a flag of the reference) the opt-in reduced-precision mode: plain bf16 operands and bf16 block-boundary "
                        "tensors in the eps-net's blocks and the priors' GEMM-shaped convolutions, tolerance 3e-2 rel-L2 against the fp32 path; default: fp32-equivalent arithmetic")
    p.add_argument("--split", choices=("f16x2", "bf16x3"), default=None,
                   help="(not a flag of the reference) the fp32-equivalent operand split of the matrix-core kernels: f16x2 (default; fp32-"
                        "equivalent inside the fp16 window 2^-6 <= |activation| < 4094) or bf16x3 (the exact three-way bf16 split, no window)")
    p.add_argument("--audit-range", action="store_true",
                   help="(not a flag of the reference) audit every f16x2 pass on the device: a geometry with a tensor wholly below the fp16 "
                        "window is repeated on bf16x3, like one that overflowed it")
    p.add_argument("--batch", type=int, default=1,
                   help="(not a flag of the reference) --generate: enhance this many files per pass as exact ragged batches - every file's "
                        "result and noise are those of the one-file loop (priors GCRN and DiffUNet); default 1: one file per pass")
    p.add_argument("--masked-prior", action="store_true",
                   help="(not a flag of the reference) --generate --batch N with a DB-AIAT prior (aia_complex_trans_ri, "
                        "dual_aia_trans_merge_crm): record the ragged batches with the length-masked attention, GRU, GroupNorm and AHAM "
                        "kernels, so that every file's result is that of the one-file loop; default: these priors refuse --batch")
    p.add_argument("--inflight", type=int, default=1,
                   help="(not a flag of the reference) --generate: keep this many files (2 .. 4) in flight on HIP streams of their own, each "
                        "verified on the device without a device-wide synchronisation (ComplexDDPMTrainer.enhance_stream); same files, "
                        "same noise; not with --batch or --audit-range; default 1: one file at a time")
    p.add_argument("--all-wav", action="store_true",
                   help="(not a flag of the reference) --generate: also read 24-bit PCM, IEEE float, G.711 A-law / mu-law and "
                        "WAVE_FORMAT_EXTENSIBLE files (up to 8 channels on the device); default: 8/16/32-bit integer PCM, other "
                        "files are skipped with a warning")
    p.add_argument("--keep-format", action="store_true",
                   help="(not a flag of the reference) --generate: write every file at its source's rate, length and channel count, in "
                        "its source's encoding (16/24/32-bit PCM, float as binary32, 8-bit and G.711 as 16-bit PCM; every channel "
                        "carries the enhanced mono signal), encoded on the device; clipped files are logged; default: 16 kHz, 16-bit, mono")
    p.add_argument("--per-channel", action="store_true",
                   help="(not a flag of the reference) --generate: enhance every channel of a file with 2 .. 8 channels on its own "
                        "(its own noise, one exact ragged pass per file; the DB-AIAT priors need --masked-prior) and write the file "
                        "with that many different channels - at 16 kHz, 16-bit, or with --keep-format in the source's rate and "
                        "encoding; mono files are untouched; default: the network enhances the mono mix")
    p.add_argument("--objective", action="store_true",
                   help="(not a flag of the reference) --eval: instead of the validation epoch, evaluate the denoising objective on the "
                        "pairs of --data / --clean - the reference's ddpm_loss, dis_loss and loss_sum with both networks in eval "
                        "mode, and ddpm_loss by diffusion step; written to objective.json")
    p.add_argument("--draws", type=int, default=1,
                   help="(not a flag of the reference) --eval --objective: evaluate every batch this many times, each with a fresh "
                        "diffusion step per utterance and fresh noise; default 1")
    p.add_argument("--members", type=int, default=1,
                   help="(not a flag of the reference) a posterior ensemble: this many (2 .. 16) reverse trajectories per utterance behind "
                        "one pass of the front end and the prior.  --generate: every file is written from the ensemble mean and "
                        "ensemble.json holds its relative spread and medoid member; --eval: the mean is scored and eval.json gains "
                        "the members' losses and the spread; not with --batch (--generate), --inflight, --per-channel, --audit-range "
                        "or --objective; default 1: one trajectory")
    p.add_argument("--window", type=int, nargs="?", const=longplan.DEFAULT_WINDOW, default=None, metavar="FRAMES",
                   help="(not a flag of the reference) --generate: recordings of any length - a file of more than FRAMES frames (10 ms "
                        "each) runs both networks in windows of FRAMES frames through one plan that every file reuses, with the result "
                        "of the whole-file pass (priors GCRN and DiffUNet); a multiple of 32, above the eps-net's receptive field of "
                        "388 + 378 frames; given without a value: %d (20.5 s; 1.6 frames computed per frame kept); not with --batch, "
                        "--inflight, --per-channel, --members, --audit-range, --eval or --objective; default: one plan per length"
                        % longplan.DEFAULT_WINDOW)
    args = p.parse_args(argv)
    if args.window is not None:
        try:
            longplan.window_arg(args.window)
        except ValueError as e:
            p.error("--window: %s" % e)
        for on, flag in ((not args.generate, "--eval" if args.eval else "anything but --generate"), (args.batch > 1, "--batch"),
                         (args.inflight > 1, "--inflight"), (args.per_channel, "--per-channel"), (args.members > 1, "--members"),
                         (args.audit_range, "--audit-range"), (args.objective, "--objective")):
            if on:
                p.error("--window with %s: windowed passes enhance one file, one trajectory at a time" % flag)
    if args.objective and not args.eval:
        p.error("--objective evaluates a held-out set: it needs --eval")
    if args.draws < 1:
        p.error("--draws must be at least 1")
    import sys

    given = sys.argv[1:] if argv is None else list(argv)
    if not 1 <= args.members <= 16:
        p.error("--members must be 1 .. 16")
    if args.members > 1:
        if args.objective:
            p.error("--objective --members: the objective plan runs one eps-net step, not a sampler to draw members from")
        for on, flag in ((args.generate and args.batch > 1, "--batch"), (args.inflight > 1, "--inflight"), (args.per_channel, "--per-channel"),
                         (args.audit_range, "--audit-range")):
            if on:
                p.error("--members with %s: ensembles are built for one file per pass, verified by its own check" % flag)
    # --eval: --batch is the validation batch size where it was given; else config.train.batch_size
    args.eval_batch = args.batch if any(a == "--batch" or a.startswith("--batch=") for a in given) else None
    args.log = os.path.join(args.assets, "log", args.doc)
    args.checkpoint = os.path.join(args.assets, "checkpoint", args.doc)
    args.generated_wav = os.path.join(args.assets, "wav", args.doc)
    with open(os.path.join("conf", args.config), "r") as f:
        config = dict2namespace(yaml.safe_load(f))
    level = getattr(logging, args.verbose.upper(), None)
    if not isinstance(level, int):
        raise ValueError("level {} not supported".format(args.verbose))  # main.py:50-51
    for d in (args.log, args.checkpoint, args.generated_wav):
        os.makedirs(d, exist_ok=True)
    logging.basicConfig(level=level, format="%(levelname)s - %(filename)s - %(asctime)s - %(message)s",
                        handlers=[logging.StreamHandler(), logging.FileHandler(os.path.join(args.log, "stdout.txt"))])
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(args.seed)
    return args, config


def main(argv=None):
    from .trainer import ComplexDDPMTrainer

    args, config = parse_args_and_config(argv)
    if args.trainer != "ComplexDDPMTrainer":
        raise NotImplementedError("only ComplexDDPMTrainer's sampling path is built")
    trainer = ComplexDDPMTrainer(args, config)
    if args.generate:
        return trainer.generate_wav(load_pre_train=True, data_path=args.data, batch=args.batch, inflight=args.inflight, members=args.members,
                                    window=args.window)
    res = trainer.train_ddpm()          # --eval: one validation epoch, or with --objective one of the denoising objective (raises NotImplementedError otherwise: training)
    import json

    with open(os.path.join(args.log, "objective.json" if args.objective else "eval.json"), "w") as f:
        json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
