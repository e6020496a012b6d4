"""The chunked form of the grouped-LSTM wavefront (pdse_glstm_desc.tc >= 1; csrc/lstm.hip: glstm_wave_kernel<NS, true> and
glstm_proj_kernel): its case table, its descriptor builder on top of helpers/lstm_cases.build, and a numpy restatement of
the form itself - the launch sequence, the lag, the ring indexing and the LayerNorm fold - shared by
tests/test_glstm_chunk_host.py (CPU) and tests/test_gpu_glstm_chunk.py.

Shapes: the smallest at which the form can go wrong, TC = 4 to reach the chunk boundaries cheaply and TC = 32 once:
  (1, 1) single frame; (2, 3) T < TC; (3, 4) T == TC; (2, 5) one frame in the last chunk; (3, 9) three chunks, both ring
  halves reused; (33, 6) two batch tiles with a padded tail in the second; (32, 33) at TC = 32, the default chunk length.
Regimes n01 (plain), offset and flat of lstm_cases: the last two broke the LayerNorm fold before it subtracted k.

The restatement keeps every ring NaN-filled until a stage stores into it, so a wrong slot or a stage that runs too early
shows as NaN in y."""
import math

import numpy as np

import emu
from helpers import lstm_cases as G

G_, H = G.G_, G.H
SHAPES = [(1, 1, 4), (2, 3, 4), (3, 4, 4), (2, 5, 4), (3, 9, 4), (33, 6, 4), (32, 33, 32)]
REGIMES = ("n01", "offset", "flat")


def _case(B, T, tc, regime, n):
    c = G._c("glstm", B=B, Bp=(B + 31) // 32 * 32, T=T, regime=regime, slices=1 + n % 2, layout=("cat", "il")[n // 2 % 2])
    c["tc"] = tc
    c["id"] += "_tc%d" % tc
    return c


CASES = [_case(B, T, tc, reg, i + j) for i, (B, T, tc) in enumerate(SHAPES) for j, reg in enumerate(REGIMES)]


def find(name):
    return next(c for c in CASES if c["id"] == name)


def scratch(case, device):
    """lstm_cases.scratch with hT1, gx2 and part as rings of R = 2 tc frames, every byte NaN."""
    R, Bp = 2 * case["tc"], case["Bp"]
    s = G.scratch(case, device)
    s.update(hT1=G._nanbuf(R * G_ * H * Bp, device), gx2=G._nanbuf(R * G_ * 4 * H * Bp, device),
             part=G._nanbuf(R * G_ * (H // 8) * Bp * 2, device))
    return s


def build(case, device, pad_nan=False, scr=None):
    b = G.build(case, device, pad_nan=pad_nan, scr=scr if scr is not None else scratch(case, device))
    b.desc.tc, b.desc.lag = case["tc"], case["tc"] + 1
    return b


def ring_h1(built, t):
    """h1[t] as the launch left it in the hT1 ring: the whole slot (t + 1) % R, padded items included."""
    c = built.case
    n = G_ * H * c["Bp"]
    slot = (t + 1) % (2 * c["tc"])
    return built.scr["hT1"].detach().cpu()[slot * n:(slot + 1) * n].clone()


def pingpong_h1(built, t):
    """h1[t] in the three-stage wavefront's ping-pong: parity (t + 1) & 1."""
    n = G_ * H * built.case["Bp"]
    slot = (t + 1) & 1
    return built.scr["hT1"].detach().cpu()[slot * n:(slot + 1) * n].clone()


def launches(T, tc):
    """The launch sequence of the chunked form: ("step", s) runs layer 1 at frame s and layer 2 at frame s - (tc + 1),
    ("proj", t0, nf) the projection of frames t0 .. t0 + nf - 1.  A projection follows its chunk's last layer-1 frame."""
    out = []
    for s in range(T + tc + 1):
        if 0 < s <= T and (s % tc == 0 or s == T):
            t0 = (s - 1) // tc * tc
            out.append(("proj", t0, s - t0))
        if s >= T and s < tc + 1:
            continue                                      # T < lag: neither stage has a frame
        out.append(("step", s))
    return out


def run_chunk(d, mem):
    """pdse_glstm_desc with tc >= 1, from the packed operands, launch by launch (own items only)."""
    Hh, Gg, T, Bp, B, TC = d.H, d.G, d.T, d.Bp, d.B, d.tc
    assert TC >= 1 and d.lag == TC + 1
    R = 2 * TC
    f = np.float32
    gx1 = mem.arr(d.gx1, Gg * T * 4 * Hh * Bp).reshape(Gg, T, Bp, 4 * Hh)
    n = Gg * (Hh // 8) * (Hh // 8) * 256
    W1 = [emu._unpack_lstm_slices(w, Hh, Hh) for w in mem.arr(d.whh1, n).reshape(Gg, -1)]
    W2 = [emu._unpack_lstm_slices(w, Hh, Hh) for w in mem.arr(d.whh2, n).reshape(Gg, -1)]
    Wi = [emu._unpack_lstm_slices(w, Hh, Hh) for w in mem.arr(d.wih2, n).reshape(Gg, -1)]
    r2, c2 = mem.arr(d.r2, Gg * 4 * Hh).reshape(Gg, 4 * Hh), mem.arr(d.c2, Gg * 4 * Hh).reshape(Gg, 4 * Hh)
    yflat, yoff = mem.view(d.y)

    def cell(gate, c):
        i_, f_, g_, o_ = np.split(gate, 4, axis=1)
        c = emu._sig(f_) * c + emu._sig(i_) * np.tanh(g_)
        return (emu._sig(o_) * np.tanh(c)).astype(f), c

    h1 = np.full((R, Gg, B, Hh), math.nan, f)             # h1[t] in slot (t + 1) % R
    gx2 = np.full((R, Gg, B, 4 * Hh), math.nan, f)        # frame t in slot t % R: chunk t // TC in half (t // TC) & 1
    c1, c2s = np.zeros((Gg, B, Hh), f), np.zeros((Gg, B, Hh), f)
    h2 = np.zeros((Gg, B, Hh), f)
    korder = [np.empty(Hh, np.int64) for _ in range(Gg)]  # stage B's K order: (source group, unit) of every position
    for g in range(Gg):
        for gq in range(Hh // 8):
            gs, kq = gq >> 5, (Hh // 16) * g + (gq & 31)
            for i in range(4):
                for hh in range(2):
                    korder[g][2 * (4 * gq + i) + hh] = gs * Hh + 8 * kq + 2 * i + hh
    for op in launches(T, TC):
        if op[0] == "proj":
            for t in range(op[1], op[1] + op[2]):
                y1 = h1[(t + 1) % R]
                mu, rs = emu._wave_moments(y1, d.eps)
                k0 = y1[0][:, 0]
                muk = (mu - k0.astype(np.float64)).astype(f)
                both = np.concatenate([y1[0], y1[1]], axis=1)                    # [B, 2H]: (source group, unit)
                for g in range(Gg):
                    xk = both[:, korder[g]]
                    gx2[t % R, g] = (rs[:, None] * ((xk - k0[:, None]) @ Wi[g].T - muk[:, None] * r2[g][None, :]) + c2[g][None, :]).astype(f)
            continue
        s = op[1]
        if s < T:                                          # stage A, frame s
            prev = np.zeros((Gg, B, Hh), f) if s == 0 else h1[s % R].copy()
            for g in range(Gg):
                h1[(s + 1) % R, g], c1[g] = cell(gx1[g, s, :B, :] + prev[g] @ W1[g].T, c1[g])
        t = s - d.lag
        if 0 <= t < T:                                     # stage C, frame s - lag
            for g in range(Gg):
                h2[g], c2s[g] = cell(gx2[t % R, g] + h2[g] @ W2[g].T, c2s[g])
                idx = (yoff + np.arange(B)[:, None] * d.y_sb + t * d.y_st + np.arange(Hh)[None, :] * d.y_su + g * d.y_sg)
                yflat[idx] = h2[g]
