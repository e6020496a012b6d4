"""Case tables and descriptor builders shared by tests/test_misc_refs_host.py (CPU tensors, replayed on tests/emu.py) and
tests/test_gpu_misc_ops.py (csrc/misc.hip: gcrnlast_kernel, time_embed_kernel, wavprep_kernel, ola_kernel, maskloss_*),
so that the two cannot drift apart.

``build(case, device)`` turns a case into one descriptor.  Every float input sits between NaN margins (a read outside its
extent poisons the result), and so does what an utterance does not own where the kernel is to skip it (frames beyond
nframes[b], spectrogram frames beyond frames[b]).  Every output sits in a NaN-filled allocation: after the launch exactly the
addressed elements are finite and everything else is NaN bit for bit (read_f / read_plane / read_d).

gcrnlast: the descriptor comes from packing.gcrn_last_fields on a synthetic state dict (decoder 2: conv1_t_2, bn1_t_2, fc2), so
the packer of the Linear's B operand is under test; out is offset by one channel plane of a [B,2,T,161] allocation with
out_sb = 2 T 161, as nets.GcrnPlan records it for decoder 2, and plane 0 must stay NaN."""
import math
import os
import zlib

import numpy as np
import torch

from conftest import pkg, rel_l2
from helpers import misc_refs as R
from helpers.tcm_cases import FM, Built, _fbuf, fptr, read_f, untouched_f  # noqa: F401  (one margin convention for all operator files)

F32, F64 = torch.float32, torch.float64
NANBITS = torch.full((1,), math.nan).view(torch.int32)
GF, GFI = 161, 80


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def by_id(cases):
    return [c["id"] for c in cases]


def find(name):
    return next(c for c in ALL if c["id"] == name)


# ---- gcrnlast ---------------------------------------------------------------------------------------------------------------
# B x T: one row (its pair partner fetches row 0); below a tile, odd, batch boundaries inside; exactly one tile; a second tile
# of one row; full tiles; 16419 rows = 514 tiles: the smallest count that gives workgroups 0 and 1 of the 512 a second trip of the
# tile loop and leaves a ragged last tile (3 rows, its last pair fetching row 0 for the row beyond the end).
GCRN_GRID_CAP = 512       # csrc/misc.hip: pdse_gcrnlast_launch
GCRN = [dict(kernel="gcrnlast", id="gl_B1_T1", B=1, T=1, bn="pos"),
        dict(kernel="gcrnlast", id="gl_B3_T7", B=3, T=7, bn="neg"),
        dict(kernel="gcrnlast", id="gl_B1_T32", B=1, T=32, bn="zero"),
        dict(kernel="gcrnlast", id="gl_B3_T11", B=3, T=11, bn="pos"),
        dict(kernel="gcrnlast", id="gl_B2_T48", B=2, T=48, bn="neg"),
        dict(kernel="gcrnlast", id="gl_B3_T5473", B=3, T=5473, bn="pos")]
GCRN_BIG = GCRN[-1]


def gcrn_ntiles(case):
    return (case["B"] * case["T"] + 31) // 32


def gcrn_params(case):
    """Natural parameters of the tail (misc_refs.gcrn_tail), float32: the three taps of w1 / w2 independent; gate weights of
    order one, so that over 64 products the logits g + b2 run from O(1) to about +-40; O(1) biases and BatchNorm shift; the
    BatchNorm scale positive, negative or exactly zero; a dense Linear."""
    g = _gen("par:" + case["id"])
    randn = lambda *s: torch.randn(*s, generator=g, dtype=F32)                             # noqa: E731
    bn_w = {"pos": 1.3, "neg": -1.1, "zero": 0.0}[case["bn"]]
    return dict(w1=randn(32, 3) * 0.25, w2=randn(32, 3), b1=float(randn(1)[0]) + 0.5, b2=float(randn(1)[0]) - 0.7,
                bn_w=bn_w, bn_b=0.5, bn_mean=0.3, bn_var=0.8, fc=randn(GF, GF) / math.sqrt(GF), fcb=randn(GF) * 0.5)


def gcrn_state_dict(p, br=2):
    """The tail's parameters under the keys of a GCRN state dict (model/gcrn.py: conv1_t_<br>, bn1_t_<br>, fc<br>)."""
    one = lambda v: torch.tensor([v], dtype=F32)                                          # noqa: E731
    q = "conv1_t_%d" % br
    return {q + ".conv1.weight": p["w1"].reshape(32, 1, 1, 3), q + ".conv1.bias": one(p["b1"]),
            q + ".conv2.weight": p["w2"].reshape(32, 1, 1, 3), q + ".conv2.bias": one(p["b2"]),
            "bn1_t_%d.weight" % br: one(p["bn_w"]), "bn1_t_%d.bias" % br: one(p["bn_b"]),
            "bn1_t_%d.running_mean" % br: one(p["bn_mean"]), "bn1_t_%d.running_var" % br: one(p["bn_var"]),
            "fc%d.weight" % br: p["fc"], "fc%d.bias" % br: p["fcb"]}


def _build_gcrn(c, device, out):
    L, P = pkg("_lib"), pkg("packing")
    B, T = c["B"], c["T"]
    g = _gen(c["id"])
    p = out.params = gcrn_params(c)
    in0 = torch.nn.functional.elu(torch.randn(B, 16, T, GFI, generator=g, dtype=F32))     # the decoder half: its producer's ELU applied
    in1 = torch.rand(B, 16, T, GFI, generator=g, dtype=F32) * 35.0 - 30.0                 # the skip half: -30 .. +5, ELU still to come
    out.in0, out.in1 = in0, in1
    f = out.fields = P.gcrn_last_fields(gcrn_state_dict(p), "conv1_t_2", 2)
    d = L.GcrnLastDesc()
    n_in = B * 16 * T * GFI
    out.in0buf, out.in1buf = _fbuf(in0, n_in, device), _fbuf(in1, n_in, device)
    out.outbuf = _fbuf(None, B * 2 * T * GF, device)
    out.keep += [out.in0buf, out.in1buf, out.outbuf]
    for k, v in f.items():
        if isinstance(v, np.ndarray):
            n = int(np.prod(v.shape))
            t = _fbuf(np.ascontiguousarray(v, np.float32), n, device)
            out.keep.append(t)
            setattr(d, k, fptr(t))
        else:
            setattr(d, k, v)
    d.in0, d.in1 = fptr(out.in0buf), fptr(out.in1buf)
    d.out, d.out_sb = fptr(out.outbuf) + 4 * T * GF, 2 * T * GF                            # decoder 2: the second channel plane
    d.B, d.T = B, T
    out.desc = d
    cache = {}

    def ref(dtype):
        if dtype not in cache:
            cache[dtype] = R.gcrn_tail(in0, in1, p, dtype)
        return cache[dtype]

    out.ref = ref


def read_plane(buf, B, T, plane=1):
    """[B,T,161] of channel plane ``plane`` of the [B,2,T,161] allocation: finite; the other plane and the margins NaN bit for bit."""
    flat = buf.detach().cpu()
    n = B * 2 * T * GF
    edge = torch.cat([flat[:FM], flat[FM + n:]]).view(torch.int32)
    assert bool((edge == NANBITS).all()), "stored outside the tensor"
    body = flat[FM:FM + n].reshape(B, 2, T, GF)
    assert bool((body[:, 1 - plane].contiguous().view(torch.int32) == NANBITS).all()), "stored into the other decoder's plane"
    got = body[:, plane]
    assert bool(torch.isfinite(got).all()), "%d elements not finite (not stored, or poisoned from a margin)" % int((~torch.isfinite(got)).sum())
    return got.clone()


# ---- time_embed -------------------------------------------------------------------------------------------------------------
def _tvals(ms):
    """0, a half step, a lerp inside, an integral step, the last row, just below it.  max_steps 50: the issue's values; a shorter
    table takes the same kinds inside its own range (the reference has no row 10 or 17 of a 7-row table to read)."""
    mid, whole = (10.45, 17.0) if ms > 17 else (ms - 3.55, float(ms - 2))
    return [0.0, 0.5, mid, whole, float(ms - 1), ms - 1 - 2.0 ** -10]


def _time_cases():
    out, k = [], {50: 0, 7: 0}
    for i, (NF, B, ms, temb) in enumerate([(0, 1, 50, True), (1, 3, 50, True), (64, 1, 7, False), (512, 3, 50, False),
                                            (513, 1, 50, True), (1000, 3, 7, True), (1024, 1, 50, False), (1500, 3, 50, True),
                                            (100, 3, 7, True), (768, 3, 50, False)]):
        tv = _tvals(ms)
        out.append(dict(kernel="time", id="te_NF%d_B%d_ms%d%s" % (NF, B, ms, "" if temb else "_notemb"), NF=NF, B=B, ms=ms, temb=temb,
                        t=[tv[(k[ms] + j) % 6] for j in range(B)]))
        k[ms] += B
    return out


TIME = _time_cases()
# finite steps outside the table: lo / hi are clamped (csrc/misc.hip), the results are those of t = 0 and t = max_steps - 1 bit for bit
TIME_OOR = [dict(kernel="time", id="te_oor_ms%d" % ms, NF=513, B=2, ms=ms, temb=True, t=[-3.5, ms + 10.25], clamped=[0.0, float(ms - 1)])
            for ms in (50, 7)]


def time_params(case):
    """nn.Linear's own initial scale, U(-1/sqrt(in), 1/sqrt(in)), for the two layers and the folded stage biases."""
    g = _gen("par:" + case["id"])
    u = lambda n, *s: (torch.rand(*s, generator=g, dtype=F32) * 2 - 1) / math.sqrt(n)     # noqa: E731
    return dict(w1=u(128, 512, 128), b1=u(128, 512), w2=u(512, 512, 512), b2=u(512, 512), wf=u(512, case["NF"], 512), bf=u(512, case["NF"]))


def _build_time(c, device, out):
    L = pkg("_lib")
    B, NF, ms = c["B"], c["NF"], c["ms"]
    p = out.params = time_params(c)
    table = out.table = R.time_table(ms)
    t = out.t = torch.tensor(c["t"], dtype=F32)
    d = L.TimeDesc()

    def put(a):
        a = torch.as_tensor(a, dtype=F32).contiguous()
        buf = _fbuf(a, a.numel(), device)
        out.keep.append(buf)
        return fptr(buf)

    d.t, d.table = put(t), put(table)
    d.p1T, d.b1, d.p2T, d.b2 = put(p["w1"].T), put(p["b1"]), put(p["w2"].T), put(p["b2"])     # transposed: thread j streams column j
    if NF:
        d.wfT, d.bf = put(p["wf"].T), put(p["bf"])
    out.outbuf = _fbuf(None, B * NF, device)
    out.tembbuf = _fbuf(None, B * 512, device)
    out.keep += [out.outbuf, out.tembbuf]
    d.out = fptr(out.outbuf)
    if c["temb"]:
        d.temb = fptr(out.tembbuf)
    d.B, d.NF, d.max_steps = B, NF, ms
    out.desc = d
    out.ref = lambda dtype: R.time_embed(t, table, p, dtype)


# ---- wavprep ----------------------------------------------------------------------------------------------------------------
AMPS = (0.05, 1.0, 20.0)
WAV_DEFAULTS = dict(kernel="wavprep", B=3, pad=160, normalize=1, c=True, lens=None, own=False)


def _w(name, **kw):
    return dict(WAV_DEFAULTS, id=name, **kw)


WAVPREP = [_w("wp_L161", L=161), _w("wp_L1000", L=1000), _w("wp_L1024_raw", L=1024, B=1, normalize=0), _w("wp_L1025_noc", L=1025, c=False),
           _w("wp_L4097", L=4097), _w("wp_L1000_pad0", L=1000, pad=0), _w("wp_L1_pad0", L=1, pad=0, B=1),
           _w("wp_lens_L1025", L=1025, lens=(0, 700, 1075)),                        # RMS length only: 0 clamps to 1, 1075 to L
           _w("wp_lens_L4097_raw", L=4097, lens=(5000, 1, 2048), normalize=0),
           _w("wp_own_L4097", L=4097, lens=(161, 2000, 4097), own=True),            # pad + 1, a middle value, L
           _w("wp_own_L1025_raw_noc", L=1025, lens=(161, 600, 1025), own=True, normalize=0, c=False),
           _w("wp_own_L1024", L=1024, lens=(1024, 161, 1023), own=True),
           _w("wp_own_nolens_L1000", L=1000, own=True)]                             # the flag without a table: the dense form


def _build_wavprep(c, device, out):
    L = pkg("_lib")
    B, Ln, pad = c["B"], c["L"], c["pad"]
    g = _gen(c["id"])
    x = out.x = torch.randn(B, Ln, generator=g, dtype=F32) * torch.tensor(AMPS[:B], dtype=F32)[:, None]
    lens = out.lens = list(c["lens"]) if c["lens"] is not None else None
    d = L.WavprepDesc()
    out.wavbuf = _fbuf(x, B * Ln, device)
    out.xpadbuf = _fbuf(None, B * (Ln + 2 * pad), device)
    out.cbuf = _fbuf(None, B, device)
    out.keep += [out.wavbuf, out.xpadbuf, out.cbuf]
    d.wav, d.xpad = fptr(out.wavbuf), fptr(out.xpadbuf)
    if c["c"]:
        d.c = fptr(out.cbuf)
    if lens is not None:
        lt = torch.tensor(lens, dtype=torch.int32).to(device)
        out.keep.append(lt)
        d.lens = lt.data_ptr()
    d.B, d.L, d.pad, d.normalize, d.reflect_own = B, Ln, pad, c["normalize"], int(c["own"])
    out.desc = d
    out.ref = lambda dtype: R.wavprep(x, pad, c["normalize"], lens, c["own"], dtype)


def own_len(case, b):
    """Samples utterance b is reflected over."""
    if case["own"] and case["lens"] is not None:
        return min(max(case["lens"][b], case["pad"] + 1), case["L"])
    return case["L"]


# ---- ola --------------------------------------------------------------------------------------------------------------------
OLA_DEFAULTS = dict(kernel="ola", B=3, n_fft=320, hop=160, cut=0, c=True, nframes=None, lens=None, zero_w0=False)


def _o(name, **kw):
    c = dict(OLA_DEFAULTS, id=name, **kw)
    c["L"] = (c["T"] - 1) * c["hop"] - c["cut"]
    for k in ("nframes", "lens"):
        if c[k] is not None:
            c[k] = tuple(c[k](c) if callable(c[k]) else c[k])
            c["B"] = len(c[k])
    return c


OLA = [_o("ola_320_T2", T=2), _o("ola_320_T3_noc", T=3, c=False), _o("ola_320_T9", T=9),
       _o("ola_320_T2_cut37", T=2, cut=37, c=False), _o("ola_320_T3_cut37", T=3, cut=37), _o("ola_320_T9_cut37", T=9, cut=37),
       _o("ola_8_2_T9", T=9, n_fft=8, hop=2),                                        # four frames overlap per sample
       _o("ola_10_4_T7", T=7, n_fft=10, hop=4, c=False),                             # the hop does not divide n_fft
       _o("ola_8_8_T5_w0", T=5, n_fft=8, hop=8, zero_w0=True),                       # zero envelope at every eighth sample: 0, not NaN
       _o("ola_320_T9_nframes", T=9, nframes=lambda c: (0, 1, c["T"], c["T"] + 5)),
       _o("ola_320_T9_lens", T=9, lens=lambda c: (0, c["L"] // 2 + 7, c["L"]), c=False),
       _o("ola_320_T9_cut37_both", T=9, cut=37, nframes=lambda c: (1, 0, 14, 5, 9), lens=lambda c: (c["L"], 300, 0, c["L"] // 2, c["L"])),
       _o("ola_8_2_T9_both", T=9, n_fft=8, hop=2, nframes=lambda c: (9, 4, 0), lens=lambda c: (16, 9, 16)),
       _o("ola_10_4_T7_nframes", T=7, n_fft=10, hop=4, nframes=lambda c: (12, 3, 1))]


def _build_ola(c, device, out):
    L = pkg("_lib")
    B, T, Ln, n_fft, hop = c["B"], c["T"], c["L"], c["n_fft"], c["hop"]
    g = _gen(c["id"])
    win = torch.hann_window(n_fft, periodic=True, dtype=F64)
    win2 = (win * win).to(F32)
    if c["zero_w0"]:
        win2[0] = 0.0
    # frames as an inverse transform leaves them: the squared window over a signal, each frame with its own deviation from it
    # (a frame taken for another, or left out, shows), so the quotient stays O(1) where a single window edge is the envelope
    sig = torch.randn(B, n_fft + hop * (T - 1), generator=g, dtype=F32)
    idx = torch.arange(n_fft)[:, None] + hop * torch.arange(T)[None, :]
    frames = win2[None, :, None] * (sig[:, idx] + 0.3 * torch.randn(B, n_fft, T, generator=g, dtype=F32))
    nfr = out.nframes = list(c["nframes"]) if c["nframes"] is not None else None
    lens = out.lens = list(c["lens"]) if c["lens"] is not None else None
    out.frames = frames.clone()
    if nfr is not None:                                                              # frames an utterance does not own: never read
        for b, n in enumerate(nfr):
            frames[b, :, min(max(n, 0), T):] = math.nan
    cs = out.c = (torch.rand(B, generator=g, dtype=F32) + 0.5) if c["c"] else None
    d = L.OlaDesc()
    out.framesbuf, out.winbuf = _fbuf(frames, B * n_fft * T, device), _fbuf(win2, n_fft, device)
    out.outbuf = _fbuf(None, B * Ln, device)
    out.keep += [out.framesbuf, out.winbuf, out.outbuf]
    d.frames, d.win2, d.out = fptr(out.framesbuf), fptr(out.winbuf), fptr(out.outbuf)
    if cs is not None:
        cb = _fbuf(cs, B, device)
        out.keep.append(cb)
        d.c = fptr(cb)
    for name, v in (("nframes", nfr), ("lens", lens)):
        if v is not None:
            t = torch.tensor(v, dtype=torch.int32).to(device)
            out.keep.append(t)
            setattr(d, name, t.data_ptr())
    d.B, d.T, d.L, d.n_fft, d.hop = B, T, Ln, n_fft, hop
    out.desc = d
    out.win2 = win2
    out.ref = lambda dtype: R.ola(out.frames, win2, n_fft, hop, Ln, cs, nfr, lens, dtype)


# ---- masked MSE -------------------------------------------------------------------------------------------------------------
MASKLOSS = [dict(kernel="maskloss", id="ml_1_2_1_161", shape=(1, 2, 1, 161), frames=(1,), scale=(1.0,)),
            dict(kernel="maskloss", id="ml_3_2_9_161", shape=(3, 2, 9, 161), frames=(0, 9, 14), scale=(1e3, 1e-4, 1.0)),
            dict(kernel="maskloss", id="ml_2_3_7_5", shape=(2, 3, 7, 5), frames=(7, 3), scale=(1e-4, 1e3)),
            dict(kernel="maskloss", id="ml_2_1_40_161", shape=(2, 1, 40, 161), frames=(45, 0), scale=(1e-2, 1e3)),
            dict(kernel="maskloss", id="ml_3_2_40_161", shape=(3, 2, 40, 161), frames=(40, 17, 1), scale=(1e-4, 1.0, 1e3))]


def _dbuf(n, device):
    return torch.full((n + 2 * FM,), math.nan, dtype=F64).to(device)


def read_d(buf, n):
    """n doubles inside a NaN-filled allocation: all written and finite, the margins NaN bit for bit."""
    flat = buf.detach().cpu()
    edge = torch.cat([flat[:FM], flat[FM + n:]]).view(torch.int64)
    assert bool((edge == torch.full((1,), math.nan, dtype=F64).view(torch.int64)).all()), "stored outside the partial sums"
    got = flat[FM:FM + n]
    assert bool(torch.isfinite(got).all())
    return got.clone()


def _build_maskloss(c, device, out):
    L = pkg("_lib")
    B, C_, T, F = c["shape"]
    g = _gen(c["id"])
    label = torch.randn(B, C_, T, F, generator=g, dtype=F32)
    esti = label + torch.randn(B, C_, T, F, generator=g, dtype=F32) * torch.tensor(c["scale"], dtype=F32)[:, None, None, None]
    out.esti, out.label = esti.clone(), label.clone()
    for b, f in enumerate(c["frames"]):                                              # behind an utterance's own frames: never read
        esti[b, :, min(max(f, 0), T):] = math.nan
        label[b, :, min(max(f, 0), T):] = math.nan
    n = B * C_ * T * F
    out.estibuf, out.labelbuf = _fbuf(esti, n, device), _fbuf(label, n, device)
    out.partial, out.outbuf = _dbuf(B * L.MASKLOSS_BLOCKS, device), _fbuf(None, 1, device)
    fr = torch.tensor(c["frames"], dtype=torch.int32).to(device)
    out.keep += [out.estibuf, out.labelbuf, out.partial, out.outbuf, fr]
    d = L.MasklossDesc()
    d.esti, d.label, d.frames = fptr(out.estibuf), fptr(out.labelbuf), fr.data_ptr()
    d.partial, d.out = out.partial.data_ptr() + 8 * FM, fptr(out.outbuf)
    d.B, d.C, d.T, d.F = B, C_, T, F
    out.desc = d
    out.ref = lambda dtype=F64: R.masked_mse(out.esti, out.label, c["frames"])


ALL = GCRN + TIME + TIME_OOR + WAVPREP + OLA + MASKLOSS
_BUILDERS = dict(gcrnlast=_build_gcrn, time=_build_time, wavprep=_build_wavprep, ola=_build_ola, maskloss=_build_maskloss)


def build(case, device):
    """The case as one descriptor on ``device``: Built with desc, its buffers, keep (every tensor a pointer names) and
    ref(dtype) -> what misc_refs says the launch computes."""
    out = Built()
    out.case, out.keep = case, []
    _BUILDERS[case["kernel"]](case, device, out)
    return out


def tensors(built):
    """Every CPU tensor the descriptor may point at (tests/emu.py resolves raw pointers through these)."""
    return built.keep


# ---- tolerance --------------------------------------------------------------------------------------------------------------
def check(what, got, ref64, ref32):
    """The project's rule, unchanged: with e32 the error of the same statement evaluated in fp32 on the CPU,
    rel_l2(result, float64) <= max(4 * e32, 2e-6) over the addressed elements.  PDSE_OPS_MARGINS=<file>: the three figures of
    every check are appended there (profiles/misc_ops_margins.txt)."""
    got, ref64, ref32 = (torch.as_tensor(a).double().reshape(-1).numpy() for a in (got, ref64, ref32))
    if ref64.size == 0:
        return 0.0, 0.0
    e32 = rel_l2(ref32, ref64)                                                           # fp32 on the CPU against float64
    err = rel_l2(got, ref64)                                                             # bound: max(4 * e32, 2e-6)
    bound = max(4 * e32, 2e-6)
    line = "%-44s e %.3e  e32 %.3e  e/e32 %6.2f  bound %.3e" % (what, err, e32, err / e32 if e32 else math.inf, bound)
    print(line)
    path = os.environ.get("PDSE_OPS_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    assert np.isfinite(err) and err <= bound, (what, err, e32, bound)
    return err, e32
