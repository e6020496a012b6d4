"""float64 numpy statement of ``pdse_ensemble_stats`` (include/pdse.h), written from its definitions: the yardstick of
tests/test_gpu_ensemble.py, itself held to a second, naive formulation in tests/test_ensemble_host.py."""
import numpy as np


def ensemble_stats(members, K, frames):
    """members: fp32 [K*B,2,T,F] or [K,B,2,T,F], member-major; frames: [B] own frames.  Returns a dict:
    mean fp32 [B,2,T,F], spread fp32 [B,T,F], per_utt float64 [B,2], per_member float64 [K,B] and mean64, the double mean."""
    x = np.asarray(members, dtype=np.float32)
    x = x.reshape((K, -1) + x.shape[-3:])
    _, B, _, T, F = x.shape
    acc = np.zeros(x.shape[1:], dtype=np.float64)
    for k in range(K):                                   # member order, in double
        acc = acc + x[k].astype(np.float64)
    mean64 = acc / np.float64(K)
    d = x.astype(np.float64) - mean64[None]              # [K,B,2,T,F]
    d2 = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]      # |d_k|^2, [K,B,T,F]
    tot = np.zeros((B, T, F), dtype=np.float64)
    for k in range(K):
        tot = tot + d2[k]
    spread = np.sqrt(tot / (K - 1)).astype(np.float32) if K > 1 else np.zeros((B, T, F), dtype=np.float32)
    m2 = mean64[:, 0] * mean64[:, 0] + mean64[:, 1] * mean64[:, 1]
    per_utt, per_member = np.zeros((B, 2)), np.zeros((K, B))
    for b in range(B):
        fr = int(frames[b])
        per_utt[b, 0] = tot[b, :fr].sum()
        per_utt[b, 1] = m2[b, :fr].sum()
        for k in range(K):
            per_member[k, b] = d2[k, b, :fr].sum()
    return {"mean": mean64.astype(np.float32), "spread": spread, "per_utt": per_utt, "per_member": per_member, "mean64": mean64}


def relative_spread(per_utt, K):
    return np.sqrt(per_utt[:, 0] / (K - 1) / per_utt[:, 1])
