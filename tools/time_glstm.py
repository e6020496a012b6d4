"""Timing of the grouped-LSTM operators alone (B=32, T=401): per-frame launches (pdse_lstm_f32 x 2 + LayerNorm +
projections) against the layer wavefront (pdse_glstm_f32).  python tools/time_glstm.py
--chunk: the three-stage wavefront beside the chunked form (pdse_glstm_desc.tc) as plans that share the GPU build them
(slices 1) and with slices 2 (tc 0 is the three-stage wavefront).  One operator holds the per-step launches and the chunk projections (the LayerNorm moments
are reduced inside the projection kernel, not in a launch of their own); a kernel trace of this run tells them apart by name:
glstm_wave_kernel<NS, false> (three stages), glstm_wave_kernel<NS, true> (stages A and C), glstm_proj_kernel."""
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
nets = importlib.import_module("prior-diffuse_amd.nets")
synth = importlib.import_module("prior-diffuse_amd.synth")
L = importlib.import_module("prior-diffuse_amd._lib")


def run(fused, B=32, T=401, reps=5, persist=False, chunk=None, slices=1):
    nets.GcrnPlan.fused_glstm = fused
    nets.GcrnPlan.persist_lstm = persist
    nets.GcrnPlan.chunk_proj = bool(chunk)
    if chunk:
        nets.GcrnPlan.CHUNK_TC = int(chunk)
    p = nets.GcrnPlan(nets.Ctx("cuda:0"), synth.make_state_dict("GCRN"), B, T, exclusive=chunk is None)
    if chunk is not None and slices == 2:
        p.exclusive = True           # timing only: the form stays as chosen above, the descriptor takes slices = 2
    p.build()
    p.finish()
    p.x.normal_()
    st = torch.cuda.current_stream().cuda_stream
    res = {}
    for _ in range(reps):
        ms = p.plan.time_ops(0, len(p.descs), st)
        for (d, tag), m in zip(p.descs, ms):
            key = type(d).__name__ + (":lstm" if tag == nets.TAG_LSTM else "")
            res.setdefault(key, []).append(m)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        p.plan.run(st)
    torch.cuda.synchronize()
    tot = (time.perf_counter() - t0) / reps * 1e3
    per = {}
    for (d, tag), i in zip(p.descs, range(len(p.descs))):
        pass
    ms = p.plan.time_ops(0, len(p.descs), st)
    lstm = sum(m for (d, tag), m in zip(p.descs, ms) if tag == nets.TAG_LSTM)
    proj = sum(m for (d, tag), m in zip(p.descs, ms) if isinstance(d, L.GconvDesc) and d.Cout == 2048)
    ln = sum(m for (d, tag), m in zip(p.descs, ms) if isinstance(d, L.LnDesc))
    if chunk is not None:
        tc = int(chunk)
        nl = (T + tc + 1 + -(-T // tc)) if tc else T + 2
        print("chunk tc=%d slices=%d  B=%d T=%d: prior %.2f ms | LSTM operator %.3f ms in %d launches (%.2f us each) | input projections %.3f ms"
              % (tc, slices, B, T, tot, lstm, nl, lstm * 1e3 / nl, proj), flush=True)
        return
    print("fused=%s persistent=%s  B=%d T=%d: prior %.2f ms | recurrent ops %.3f ms (%.2f us/step) | input projections %.3f ms | LayerNorm %.3f ms"
          % (fused, bool(getattr(p, "persist", False)), B, T, tot, lstm, lstm * 1e3 / ((T + 1) if getattr(p, "persist", False) else (T + 2) if fused else 2 * T), proj, ln), flush=True)


if __name__ == "__main__":
    if "--persist" in sys.argv:      # the small-batch persistent form (csrc/lstmp.hip) beside the wavefront
        for B, T in ((1, 401), (2, 401), (4, 401), (8, 401), (1, 1001)):
            run(True, B, T)
            run(True, B, T, persist=True)
        sys.exit(0)
    if "--chunk" in sys.argv:        # the chunked form beside the three-stage wavefront, both as a shared-GPU plan builds them
        for tc in (0, 16, 32, 64):
            for sl in (1, 2):
                run(True, 32, 401, chunk=tc, slices=sl)
        sys.exit(0)
    for B, T in ((32, 401), (1, 401), (16, 1001)):
        run(False, B, T)
        run(True, B, T)
