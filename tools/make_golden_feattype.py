"""Fixture of the spectral compression modes (tests/golden/feat_type.npz) from the REFERENCE's own text.

    python tools/make_golden_feattype.py /path/to/reference

One input, a complex STFT [B = 2, 2, T = 9, 161]: seeded normal values with planted specials in frames 0 and 1 of utterance 0
(``PLANTED``: exact zeros, a zero real part, negative real parts, magnitudes 1e-30, 1e-8, 1 and 30, fp32 denormals; the bins of
magnitude 30 are Pythagorean, so their fp32 magnitude is exact and exp(30) is not fed a rounded argument).  For each of the five
feat_type values ("none" stands for the reference's "any other string") the statements are cut out of the reference's syntax
trees and compiled as they stand - the technique of tools/make_golden_validation.py - so nothing of its text enters this
repository:

  * comp_<mode>: the validation loop's compression statements (trainer/complex_ddpm_trainer.py:414-435) on the input;
  * dec_<mode>: compare_complex's decompression statements (utils/metrics.py:531-551) on the input;
  * wav_<mode>: the waveforms compare_complex hands to compareone (:552-566: torch.istft, cut to (frames - 1) * 160).

Beside them the tool measures, on the CPU, how far these fp32 results lie from the float64 restatement of
tests/helpers/feat_refs.py (rel-L2 and max-abs per transform) and writes the figures and the bounds that follow from them for the
device (twice the distance, tests/test_gpu_feat_type.py) to profiles/feat_type_parity.txt."""
import ast
import importlib
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

SEED, B, T, F = 4100, 2, 9, 161
MODES = ("sqrt", "normal", "cubic", "log_1x", "none")
# (frame, bin, re, im) in utterance 0; frames 0 and 1 only, so that the [0:1, :, 0:2] corner holds every special
PLANTED = (
    (0, 0, 0.0, 0.0), (0, 1, 0.0, 0.7), (0, 2, -1.3, 0.4), (0, 3, 1e-30, 0.0), (0, 4, 6e-31, -8e-31), (0, 5, 1e-8, 0.0),
    (0, 6, -6e-9, 8e-9), (0, 7, 1.0, 0.0), (0, 8, 0.0, -1.0), (0, 9, -0.6, 0.8), (0, 10, 30.0, 0.0), (0, 11, 18.0, 24.0),
    (0, 12, -24.0, 18.0), (0, 13, 1e-40, -3e-41), (0, 14, 1e-39, 0.0), (0, 160, 0.0, 0.0),
    (1, 0, 0.0, -30.0), (1, 1, -18.0, -24.0), (1, 2, 24.0, -18.0), (1, 3, -30.0, 0.0), (1, 4, 0.0, 0.0), (1, 5, 0.0, 1e-8),
    (1, 6, -1e-30, 1e-30), (1, 7, -1.0, 0.0), (1, 8, 0.0, 1e-42), (1, 9, -0.0, 0.0), (1, 160, -2.5, 0.0),
)


def make_input():
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(B, 2, T, F, generator=g, dtype=torch.float32) * 1.5
    for t, f, re, im in PLANTED:
        x[0, 0, t, f], x[0, 1, t, f] = re, im
    return x


def main():
    ref = sys.argv[1]
    MG = importlib.import_module("oracle.make_golden")
    R = importlib.import_module("feat_refs")
    warnings.simplefilter("ignore")
    tview = MG._LegacyTorch(None)
    x = make_input()
    # ---- the compression statements of the validation loop
    tree = ast.parse(open(ref + "/trainer/complex_ddpm_trainer.py").read())
    fn = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "train_ddpm"][0]
    loop = [n for n in ast.walk(fn) if isinstance(n, ast.For) and isinstance(n.target, ast.Name) and n.target.id == "batch"
            and "cv_dataloader" in ast.unparse(n.iter)][0]
    body = loop.body
    i0 = [i for i, st in enumerate(body) if isinstance(st, ast.Assign) and ast.unparse(st.targets[0]) == "noisy_phase"][0]
    i1 = [i for i, st in enumerate(body) if isinstance(st, ast.Assign) and ast.unparse(st.targets[0]) == "init_audio"][0]
    compression = compile(ast.Module(body=body[i0:i1], type_ignores=[]), "ref_validation_compression", "exec")
    # ---- compare_complex: its decompression statements alone, and the whole function with compareone as a recorder
    cc = MG._ast_defs(ref + "/utils/metrics.py", ["compare_complex"])[0]
    inner = [n for n in ast.walk(cc) if isinstance(n, ast.With)][0].body
    j1 = [i for i, st in enumerate(inner) if isinstance(st, ast.Assign) and "clean_utts" in ast.unparse(st.targets[0])][0]
    decompression = compile(ast.Module(body=inner[:j1], type_ignores=[]), "ref_compare_decompression", "exec")
    pairs = []
    ns3 = {"torch": tview, "np": np, "compareone": lambda cp: (pairs.append(cp), (0.0,) * 6)[1]}
    exec(compile(ast.Module(body=[cc], type_ignores=[]), "ref_compare_complex", "exec"), ns3)
    res = dict(seed=SEED, input=x.numpy(), planted=np.array(PLANTED, dtype=np.float64))
    lines = ["# fp32 statements of the reference (CPU, torch %s) against the float64 restatement of tests/helpers/feat_refs.py" % torch.__version__,
             "# input: seed %d, [%d, 2, %d, %d], %d planted bins; bound = 2 x measured (tests/test_gpu_feat_type.py)" % (SEED, B, T, F, len(PLANTED)),
             "# %-18s %12s %12s %12s %12s" % ("transform", "rel-L2", "max-abs", "bound rel-L2", "bound max-abs")]
    for mode in MODES:
        self_ = types.SimpleNamespace(config=types.SimpleNamespace(train=types.SimpleNamespace(feat_type=mode)))
        ns2 = {"self": self_, "torch": tview, "batch_feat": x.clone(), "batch_label": x.clone()}
        exec(compression, ns2)
        assert torch.equal(ns2["batch_feat"], ns2["batch_label"])
        comp = ns2["batch_label"].contiguous().numpy()
        ns4 = {"torch": tview, "esti_list": x.clone(), "label_list": x.clone(), "feat_type": mode}
        exec(decompression, ns4)
        dec = ns4["esti_com"].contiguous().numpy()
        del pairs[:]
        ns3["compare_complex"](x.clone(), x.clone(), [T] * B, feat_type=mode)
        wav = np.stack([np.asarray(p, dtype=np.float32) for _, p in pairs])
        assert comp.shape == dec.shape == (B, 2, T, F) and wav.shape == (B, (T - 1) * 160)
        res["comp_" + mode], res["dec_" + mode], res["wav_" + mode] = comp, dec, wav
        for kind, got, want in (("compress", comp, R.compress(x.numpy(), mode)), ("decompress", dec, R.decompress(x.numpy(), mode)),
                                ("wav", wav, R.wav_of(x.numpy(), mode))):
            assert np.isfinite(got).all() and np.isfinite(want).all()
            rel, mx = R.errors(got, want)
            res["err_%s_%s" % (kind, mode)] = np.array([rel, mx])
            lines.append("  %-18s %12.3e %12.3e %12.3e %12.3e" % (kind + " " + mode, rel, mx, 2 * rel, 2 * mx))
    out = os.path.join(ROOT, "tests", "golden", "feat_type.npz")
    np.savez_compressed(out, **res)
    print("\n".join(lines))
    print(out, os.path.getsize(out), "bytes")
    with open(os.path.join(ROOT, "profiles", "feat_type_parity.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
