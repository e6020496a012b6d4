"""On the GPU box: ``ComplexDDPMTrainer.objective_batch`` at the reference's training shape against the same evaluation put
together from the operators the package had before it.

    python tools/time_objective.py [--batch 8] [--seconds 3] [--runs 5] [--calls 10] [--out profiles/objective_timing.txt]

B = 8 utterances of 3 s (T = 301), GCRN prior, synthetic weights, with and without --sigma.  The composed side: the feature and
the label through ``ops.label_spec``, the prior operator, ``ops.spec_losses`` for dis_loss, two torch divisions by 11,
``ops.q_sample`` (which indexes the schedule with torch and, with sigma, runs the mask as a launch of its own), ``DiffUNet1Op``,
then ``ops.spec_losses`` or, with sigma, the loss in torch; one synchronising finiteness check at the end, as the pass's own check
synchronises.  Both sides start from waveforms that are already on the device, as the epoch's file loop hands them over.  Medians of
``--runs`` timings of ``--calls`` calls each, lowest .. highest, after two warm-up calls of each side.
Then the two new entries alone, with device events around ``--calls`` x 10 back-to-back calls of the C entries (``_lib``, no
Python argument checking in between): their time, their share of the pass and the bytes they move per second against the HBM
rate (8 TB/s peak, about 6.3 TB/s achievable).  A call that takes a few microseconds is bounded by its launches as much as by its
bytes: with sigma the noising is a memset and two kernels, the loss two kernels.  The byte counts are what the
algorithm needs: the noising reads label, init and noise and writes noisy and target (with sigma, init a second time for the
maximum), the loss reads the live frames of predicted, target and init.  At this size every tensor (3.1 MB) stays in the
256 MiB last-level cache between launches, so the rates are on-die rates, not HBM traffic."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objective_timing.txt"))
    a = ap.parse_args()
    import __graft_entry__ as ge

    ge.build()
    if not torch.cuda.is_available():
        raise RuntimeError("time_objective.py measures on the GPU; there is none here")
    pk = lambda m: importlib.import_module("prior-diffuse_amd." + m)      # noqa: E731
    synth, ops, tr, lib = pk("synth"), pk("ops"), pk("trainer"), pk("_lib")
    dev = "cuda:0"
    B, L_ = a.batch, int(a.seconds * 16000)
    T = 1 + L_ // 160
    lens = [L_] * B
    frames = [T] * B
    g = torch.Generator().manual_seed(3)
    clean = [0.05 * torch.randn(L_, generator=g) for _ in range(B)]
    noisy = [(c + 0.02 * torch.randn(L_, generator=g)).to(dev) for c in clean]
    clean = [c.to(dev) for c in clean]
    noise = torch.randn(B, 2, T, 161, generator=g).to(dev)
    steps = torch.randint(0, 50, [B], generator=g).to(dev)
    gs, ds = synth.make_state_dict("GCRN"), synth.make_state_dict("DiffUNet1")
    config = argparse.Namespace(model=argparse.Namespace(name="GCRN"),
                                train=argparse.Namespace(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt", batch_size=B))

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0) / a.calls)
        return float(np.median(ms)), min(ms), max(ms)

    def events(fn):
        n = a.calls * 10
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(a.runs):
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / n)
        return float(np.median(ms)), min(ms), max(ms)

    lines = ["tools/time_objective.py --batch %d --seconds %g --runs %d --calls %d" % (B, a.seconds, a.runs, a.calls),
             "B = %d x %.1f s (T = %d), GCRN prior, default trainer, ms per batch: medians of %d timings of %d calls (lowest .. highest)"
             % (B, a.seconds, T, a.runs, a.calls)]
    results = []

    def report(name, unit, m):
        lines.append("%-66s %8.3f %s  (%.3f .. %.3f)" % (name, m[0], unit, m[1], m[2]))
        results.append({"name": name, "unit": unit, "median": round(m[0], 4), "min": round(m[1], 4), "max": round(m[2], 4), "runs": a.runs})

    for sigma in (False, True):
        args = argparse.Namespace(retrain=False, joint=True, draw=False, sigma=sigma, checkpoint="", generated_wav="")
        t = tr.ComplexDDPMTrainer(args, config, device=dev, prior_state_dict=gs, ddpm_state_dict=ds)
        nb, cb = torch.stack(noisy), torch.stack(clean)

        def device_side():
            return t.objective_batch(noisy, clean, t=steps, noise=noise)

        def composed():
            feat, _ = ops.label_spec(nb, nb, lens)
            label, _ = ops.label_spec(nb, cb, lens)
            x_init = t.model(feat)
            dis = ops.spec_losses(x_init, label, frames)
            init, lab = x_init / 11, label / 11
            noisy_a = ops.q_sample(lab, init, steps, noise, mode="pirorgrad", sigma=sigma)
            predicted = t.model_ddpm(noisy_a, init, steps)
            if sigma:
                tmp = torch.flatten(torch.abs(init), start_dim=2)
                mask = (tmp / torch.max(tmp, dim=2, keepdim=True).values / 2 + 0.5).view(init.shape)
                d = predicted - noise * mask ** 0.5
                ddpm = (d / mask * d).sum() / (2 * 161 * sum(frames))
            else:
                ddpm = ops.spec_losses(predicted, noise, frames)["com_mag_mse"]
            if not bool(torch.isfinite(predicted).all()):
                raise RuntimeError("non-finite prediction")
            return ddpm, dis

        tag = "--sigma" if sigma else "no sigma"
        both = []
        for name, fn in (("objective_batch (%s)" % tag, device_side), ("composed from the earlier operators (%s)" % tag, composed),
                         ("objective_batch (%s), again" % tag, device_side), ("composed from the earlier operators (%s), again" % tag, composed)):
            m = timed(fn)
            both.append(m)
            report(name, "ms per batch", m)
        sc = t.objective_batch(noisy, clean, t=steps, noise=noise, tensors=True)
        cm = composed()[0]
        own = sc["ddpm"]["loss"][0 if sigma else 2]
        lines.append("    ddpm_loss of the two sides on the same inputs: %.9g and %.9g" % (float(own), float(cm)))
        pass_ms = min(both[0][0], both[2][0])
        # the new entries alone, on the pass's own tensors
        label, init, predicted, target = sc["label"], sc["init"], sc["predicted"], sc["target"]
        out = (torch.empty_like(label), torch.empty_like(label), torch.empty(2 * B, device=dev))
        n_bytes = label.numel() * 4
        a_tab, s_tab, _ = ops.noise_tables(torch.device(dev))
        t32, stream = steps.to(torch.int32), torch.cuda.current_stream().cuda_stream
        m = events(lambda: lib.objective_noise(label.data_ptr(), init.data_ptr(), noise.data_ptr(), t32.data_ptr(), a_tab.data_ptr(),
                                               s_tab.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), B, T, 161, 0,
                                               1 if sigma else 0, stream))
        assert torch.equal(out[0], sc["noisy"]) and torch.equal(out[1], target)
        moved = (6 if sigma else 5) * n_bytes
        report("pdse_objective_noise alone (%s)" % tag, "ms per call", m)
        lines.append("    %.1f MB per call -> %.2f TB/s, %.0f %% of the achievable HBM rate (%.1f TB/s; peak %.1f); %.1f %% of the pass"
                     % (moved / 1e6, moved / (m[0] * 1e-3) / 1e12, 100 * moved / (m[0] * 1e-3) / HBM_ACHIEVABLE, HBM_ACHIEVABLE / 1e12,
                        HBM_PEAK / 1e12, 100 * m[0] / pass_ms))
        if sigma:
            maxbuf = out[2].clone()
            fh = np.array(frames, dtype=np.int32)
            fd = torch.from_numpy(fh).to(dev)
            partial, per = torch.empty(B * lib.SPECLOSS_BLOCKS, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)
            loss = torch.empty(1, device=dev)
            m2 = events(lambda: lib.sigma_loss(predicted.data_ptr(), target.data_ptr(), init.data_ptr(), maxbuf.data_ptr(), fh.ctypes.data,
                                               fd.data_ptr(), partial.data_ptr(), per.data_ptr(), loss.data_ptr(), B, T, 161, stream))
            assert torch.equal(loss[0], sc["ddpm"]["loss"][0])
            report("pdse_sigma_loss alone", "ms per call", m2)
            lines.append("    %.1f MB per call -> %.2f TB/s, %.0f %% of the achievable HBM rate; %.1f %% of the pass; both entries: %.1f %% of the pass"
                         % (3 * n_bytes / 1e6, 3 * n_bytes / (m2[0] * 1e-3) / 1e12, 100 * 3 * n_bytes / (m2[0] * 1e-3) / HBM_ACHIEVABLE,
                            100 * m2[0] / pass_ms, 100 * (m[0] + m2[0]) / pass_ms))
        del t
    lines += ["RESULT " + json.dumps(r) for r in results]
    print("\n".join(lines))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
