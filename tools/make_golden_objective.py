"""Fixture of the denoising objective (tests/golden/objective_step.npz) from the REFERENCE's own text.

    python tools/make_golden_objective.py /path/to/reference

One batch of B = 3, T = 5, F = 161 with frames (5, 3, 2) and diffusion steps t = (0, 49, 17), through

  * the statements of ``train_step`` from ``batch_label /= self.c`` to the assignment of ``loss_ddpm``
    (trainer/complex_ddpm_trainer.py:699-738), with ``self.model_ddpm`` replaced by a recorder that returns a seeded stand-in
    for ``predicted``, ``torch.randint`` / ``torch.randn_like`` by the injected t and noise, and ``self.noise_level`` built by the
    constructor's own three statements (:42-44) from the reference's ``params``;
  * ``com_mse_sigma_loss``, ``com_mse_loss`` and ``com_mag_mse_loss`` of utils/loss.py, which those statements call.

The statements and functions are cut out of the reference's syntax trees and compiled as they stand - the technique of
tools/make_golden_validation.py - so nothing of the reference's text is copied into this repository.  The inputs come from
tests/helpers/objective_refs.py (seeds), where the tests regenerate them; stored are, for each of the three parameterisations
with and without --sigma, ``noisy`` and the losses (``target`` once: it does not depend on the parameterisation, and without
--sigma it is the noise itself), and ``f64_distance``: how far the float64 sum of the same fp32 terms lies from the reference's
fp32 loss (relative; printed) - the allowance of the tests is four times that.

One substitution, the one tests/test_gpu_round2.py::test_q_sample_branches_bit_exact makes: torch's vectorised CPU square root
is not correctly rounded (it differs from the IEEE result in about 0.7 % of elements, and not in the same ones under every
ATEN_CPU_CAPABILITY), while the reference's CUDA path and the HIP kernels take the IEEE square root.  The statements' three
``** 0.5`` therefore see tensors whose square root is numpy's (``_IeeeRoot``); every other operation is torch's own."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


class _IeeeRoot(torch.Tensor):
    """An fp32 tensor whose ``** 0.5`` is the correctly rounded square root.  Results of torch operations on it are of this class
    too, so ``self.noise_level[t]`` ... ``(1.0 - noise_scale) ** 0.5`` and ``torch.flatten(...)`` ... ``mask ** 0.5`` end here."""

    def __pow__(self, e):
        plain = self.as_subclass(torch.Tensor)
        return torch.from_numpy(np.sqrt(plain.numpy())) if e == 0.5 else plain ** e


class _Injected:
    """``torch`` as the extracted statements see it: ``randint`` returns the injected t, ``randn_like`` the injected noise, and
    ``flatten`` - the first operation of the --sigma mask - hands out an ``_IeeeRoot``."""

    def __init__(self, t, noise):
        self._t, self._noise, self.calls = t, noise, []

    def randint(self, *a, **kw):
        self.calls.append("randint")
        return self._t.clone()

    def randn_like(self, x):
        self.calls.append("randn_like")
        return self._noise.clone()

    def flatten(self, *a, **kw):
        return torch.flatten(*a, **kw).as_subclass(_IeeeRoot)

    def __getattr__(self, name):
        return getattr(torch, name)


def _statements(ref):
    tree = ast.parse(open(ref + "/trainer/complex_ddpm_trainer.py").read())
    init = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "__init__"][0]
    level = [st for st in init.body if isinstance(st, ast.Assign) and ast.unparse(st.targets[0]) in ("beta", "noise_level", "self.noise_level")]
    fn = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "train_step"][0]
    i0 = [i for i, st in enumerate(fn.body) if isinstance(st, ast.AugAssign) and isinstance(st.op, ast.Div)
          and ast.unparse(st.target) == "batch_label"][0]
    i1 = [i for i, st in enumerate(fn.body) if isinstance(st, ast.If) and "loss_ddpm" in ast.unparse(st.body[0])][0]
    assert len(level) == 3 and i1 > i0
    return level, fn.body[i0:i1 + 1]


def main():
    ref = sys.argv[1]
    MG = importlib.import_module("oracle.make_golden")
    MG.REF = ref
    R = importlib.import_module("helpers.objective_refs")
    warnings.simplefilter("ignore")
    params = MG._load("ref_params", ref + "/utils/params.py").params
    level, body = _statements(ref)
    label0, init0, noise, predicted = (torch.from_numpy(x) for x in R.raw_inputs())
    label, init, _, _ = R.inputs()
    t = torch.tensor(R.STEPS, dtype=torch.int64)
    frames = list(R.FRAMES)
    losses = {}
    exec(compile(ast.Module(body=MG._ast_defs(ref + "/utils/loss.py", ["com_mse_sigma_loss", "com_mse_loss", "com_mag_mse_loss"]),
                            type_ignores=[]), "ref_loss", "exec"), dict(torch=torch, nn=torch.nn, np=np), losses)
    res = dict(seed=R.SEED, frames=np.array(frames), t=np.array(R.STEPS), noise_schedule=np.array(params.noise_schedule))
    dist = {}
    for mode in R.MODES:
        for sigma, names in ((False, ("com_mse_loss", "com_mag_mse_loss")), (True, ("com_mse_sigma_loss",))):
            key = R.case_key(mode, sigma)
            for name in names:
                seen = []
                tview = _Injected(t, noise)
                self_ = types.SimpleNamespace(c=11, params=params, pirorgrad=mode == "pirorgrad", deltamu=mode == "deltamu",
                                              args=types.SimpleNamespace(sigma=sigma),
                                              config=types.SimpleNamespace(train=types.SimpleNamespace(loss=name)),
                                              model_ddpm=lambda *a: (seen.append(a), predicted.clone())[1])
                ns = dict(losses, self=self_, torch=tview, np=np, batch_label=label0.clone(), init_audio=init0.clone(),
                          batch_feat=torch.zeros_like(label0), batch_frame_num_list=frames)
                exec(compile(ast.Module(body=level, type_ignores=[]), "ref_noise_level", "exec"), ns)
                self_.noise_level = self_.noise_level.as_subclass(_IeeeRoot)
                exec(compile(ast.Module(body=body, type_ignores=[]), "ref_train_step_ddpm", "exec"), ns)
                assert tview.calls == ["randint", "randn_like"] and len(seen) == 1 and torch.equal(seen[0][-1], t)
                assert np.array_equal(ns["batch_label"].numpy(), label) and np.array_equal(ns["init_audio"].numpy(), init)
                assert torch.equal(seen[0][0], ns["noisy_audio"]) and len(seen[0]) == (2 if mode == "deltamu" else 3)
                noisy, target = ns["noisy_audio"].numpy(), ns["noise"].numpy()
                res[key + "_noisy"] = noisy
                if sigma:
                    assert "target_sigma" not in res or np.array_equal(res["target_sigma"], target)
                    res["target_sigma"] = target
                    _, mx = R.mask_of(init)
                    f64 = R.sigma_loss(predicted.numpy(), target, init, mx, frames)[1]
                else:
                    assert np.array_equal(target, noise.numpy())
                    f64 = R.spec_losses(predicted.numpy(), target, frames)[1][0 if name == "com_mse_loss" else 2]
                value = float(ns["loss_ddpm"])
                short = name[:-len("_loss")]
                res[key + "_" + short] = value
                dist[key + "_" + short] = abs(f64 - value) / value
                print("%-18s %-15s loss %.9g  float64 sum of the fp32 terms %.12g  relative distance %.3e" % (key, short, value, f64, dist[key + "_" + short]))
    res["f64_distance_keys"] = np.array(sorted(dist))
    res["f64_distance"] = np.array([dist[k] for k in sorted(dist)])
    out = os.path.join(ROOT, "tests", "golden", "objective_step.npz")
    np.savez_compressed(out, **res)
    print(out, os.path.getsize(out), "bytes (tests/golden/validation_epoch.npz: %d)"
          % os.path.getsize(os.path.join(ROOT, "tests", "golden", "validation_epoch.npz")))


if __name__ == "__main__":
    main()
