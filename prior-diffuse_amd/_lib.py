"""ctypes binding of libpdse.so (the C-ABI declared in include/pdse.h).

The product path has no CPU fallback: if the shared library is missing or does not
match the header this module raises, and so does everything built on it.
"""
import contextlib
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PDSE_LIB") or os.path.join(_HERE, "libpdse.so")   # PDSE_LIB: diagnostic builds only

ABI_VERSION = 9

ACT_NONE, ACT_PRELU, ACT_ELU, ACT_SIGMOID = 0, 1, 2, 3
EPI_LINEAR, EPI_GLU, EPI_BIGLU = 0, 1, 2
EW_DIV, EW_UPDATE, EW_UPDATE_FINAL, EW_COPY, EW_ADD_MUL = 0, 1, 2, 3, 4
(OP_GCONV, OP_TIME, OP_EW, OP_COMPAND, OP_WAVPREP, OP_OLA, OP_SIGMA, OP_LN, OP_LSTM,
 OP_ROWLN, OP_CHLN, OP_ATTN, OP_GRU, OP_GNCOMB, OP_AHAM, OP_QSAMPLE, OP_TRANSPOSE, OP_TCM, OP_CRM, OP_GCRNLAST,
 OP_MASKLOSS, OP_GLSTM, OP_TCM2, OP_BGLU, OP_PLANES, OP_GLSTMP, OP_TCM2S, OP_DENSE, OP_ROWLNB, OP_METRICS, OP_RESAMPLE, OP_RANGE) = range(32)
MASKLOSS_BLOCKS = 32
SPECLOSS_BLOCKS = 32      # PDSE_SPECLOSS_BLOCKS: workgroups per utterance of pdse_spec_losses (partial [B][32][2] doubles)

ENSEMBLE_BLOCKS = 32      # PDSE_ENSEMBLE_BLOCKS: workgroups per utterance of pdse_ensemble_stats (partial [B][32][K + 2] doubles)
ENSEMBLE_MAX = 16         # PDSE_ENSEMBLE_MAX: members of a posterior ensemble (a thread of pdse_ensemble_stats holds K values in registers)
_fp = C.c_void_p  # device pointers travel as integers
_i32, _i64, _f32 = C.c_int32, C.c_int64, C.c_float


class Src(C.Structure):
    _fields_ = [("ptr", _fp), ("sb", _i64), ("sc", _i64), ("st", _i64), ("sf", _i64),
                ("C", _i32), ("act", _i32), ("blk", _i32), ("pad_", _i32)]


class GconvDesc(C.Structure):
    _fields_ = [
        ("in0", Src), ("in1", Src),
        ("Tin", _i32), ("Fin", _i32),
        ("padrow", _fp), ("padrow_sb", _i64),
        ("taps", _fp), ("ntaps", _i32), ("sf_in", _i32),
        ("xf_scale0", _fp), ("xf_shift0", _fp), ("xf_scale1", _fp), ("xf_shift1", _fp),
        ("xf_slope0", _f32), ("xf_slope1", _f32), ("xf_mode", _i32), ("cin1", _i32),
        ("w0", _fp), ("w1", _fp), ("ksteps", _i32), ("Cout", _i32),
        ("bias0", _fp), ("bias1", _fp), ("bias0_sb", _i64), ("bias1_sb", _i64),
        ("epi", _i32), ("act", _i32), ("act_slope", _f32), ("C2", _i32),
        ("post_scale", _fp), ("post_shift", _fp),
        ("wlc", _fp), ("wrc", _fp), ("blc", _fp), ("brc", _fp), ("wc2", _fp), ("bc2", _fp),
        ("resid", _fp), ("out", _fp),
        ("out_sb", _i64), ("out_sc_hi", _i64), ("out_sc_lo", _i64), ("out_st", _i64),
        ("out_sf", _i64), ("out_off", _i64),
        ("out_cr", _i32), ("B", _i32), ("Tout", _i32), ("Fout", _i32),
        ("korder", _i32), ("ksteps1", _i32), ("w2", _fp), ("w3", _fp), ("p1mask", _i32), ("Fout1", _i32),
        ("nx_w", _fp), ("nx_bias", _fp * 3), ("nx_add", _fp * 3), ("nx_out", _fp * 3), ("nx_bias_sb", _i64 * 3),
        ("nx_sb", _i64 * 3), ("nx_sc", _i64 * 3), ("nx_st", _i64 * 3), ("nx_sf", _i64 * 3), ("nx_off", _i64 * 3),
        ("nx_n", _i32), ("nx_keep", _i32), ("nx_row0", _i32), ("wexp", _i32),
        ("bias0_t0", _fp), ("bias1_t0", _fp),
        ("tap_dt", _i32 * 12), ("tap_df", _i32 * 12), ("flat", _i32), ("pad_", _i32),
    ]


class TimeDesc(C.Structure):
    _fields_ = [("t", _fp), ("table", _fp), ("p1T", _fp), ("b1", _fp), ("p2T", _fp), ("b2", _fp),
                ("wfT", _fp), ("bf", _fp), ("out", _fp), ("temb", _fp),
                ("B", _i32), ("NF", _i32), ("max_steps", _i32), ("pad_", _i32)]


class EwDesc(C.Structure):
    _fields_ = [("a", _fp), ("b", _fp), ("c", _fp), ("out", _fp), ("n", _i64),
                ("s0", _f32), ("s1", _f32), ("s2", _f32), ("op", _i32)]


class CompandDesc(C.Structure):
    _fields_ = [("in_", _fp), ("out", _fp), ("plane", _i64), ("B", _i32), ("mode", _i32),
                ("out_sb", _i64), ("out_sc", _i64), ("out_st", _i64), ("F", _i32), ("pad_", _i32)]


# pdse_compand_desc.mode (include/pdse.h PDSE_COMPAND_*) and the feat_type values of the configuration files: what the front
# end and the label leg record (None: no launch) and what the back end and the scored waveforms decompress with
COMPAND_SQRT, COMPAND_SQUARE, COMPAND_MAG, COMPAND_COPY, COMPAND_POW03, COMPAND_POW103, COMPAND_LOG1X, COMPAND_EXPM1 = range(8)
FEAT_TYPES = ("sqrt", "normal", "cubic", "log_1x", "none")
COMPRESS_MODE = {"sqrt": COMPAND_SQRT, "normal": COMPAND_MAG, "cubic": COMPAND_POW03, "log_1x": COMPAND_LOG1X, "none": None}
DECOMPRESS_MODE = {"sqrt": COMPAND_SQUARE, "normal": COMPAND_COPY, "cubic": COMPAND_POW103, "log_1x": COMPAND_EXPM1,
                   "none": COMPAND_COPY}


def feat_type_of(value):
    """``value`` if it is one of FEAT_TYPES, else ValueError.  The reference treats every string outside its list as "leave the
    STFT alone"; here only the literal "none" means that, so that a misspelt mode does not pass for one."""
    if value not in FEAT_TYPES:
        raise ValueError("feat_type %r: must be one of 'sqrt', 'normal', 'cubic', 'log_1x', 'none'" % (value,))
    return value


def members_arg(members):
    """``members`` of the ensemble entry points as an int in 1 .. ENSEMBLE_MAX; anything else: ValueError.  Host only."""
    if isinstance(members, bool) or not isinstance(members, int) or not 1 <= members <= ENSEMBLE_MAX:
        raise ValueError("members must be an integer in 1 .. %d (pdse_ensemble_stats holds a bin's members in registers), got %r"
                         % (ENSEMBLE_MAX, members))
    return members


class WavprepDesc(C.Structure):
    _fields_ = [("wav", _fp), ("xpad", _fp), ("c", _fp), ("lens", _fp),
                ("B", _i32), ("L", _i32), ("pad", _i32), ("normalize", _i32), ("reflect_own", _i32), ("pad_", _i32)]


class OlaDesc(C.Structure):
    _fields_ = [("frames", _fp), ("win2", _fp), ("c", _fp), ("out", _fp),
                ("B", _i32), ("T", _i32), ("L", _i32), ("n_fft", _i32), ("hop", _i32), ("pad_", _i32),
                ("nframes", _fp), ("lens", _fp)]


class SigmaDesc(C.Structure):
    _fields_ = [("init", _fp), ("a", _fp), ("out", _fp), ("maxbuf", _fp), ("plane", _i64),
                ("nplanes", _i32), ("pad_", _i32), ("valid", _fp)]


class LnDesc(C.Structure):
    _fields_ = [("in_", _fp), ("gamma", _fp), ("beta", _fp), ("out", _fp),
                ("osb", _i64), ("os_hi", _i64), ("os_lo", _i64), ("os_t", _i64),
                ("B", _i32), ("T", _i32), ("N", _i32), ("r", _i32), ("eps", _f32), ("blk", _i32)]


class LstmDesc(C.Structure):
    _fields_ = [("gx", _fp), ("whh", _fp), ("hT", _fp), ("cst", _fp), ("y", _fp),
                ("y_sb", _i64), ("y_st", _i64), ("y_su", _i64), ("y_sg", _i64),
                ("B", _i32), ("Bp", _i32), ("T", _i32), ("H", _i32), ("G", _i32), ("pad_", _i32)]


class GlstmDesc(C.Structure):
    _fields_ = [("gx1", _fp), ("whh1", _fp), ("wih2", _fp), ("r2", _fp), ("c2", _fp), ("whh2", _fp),
                ("hT1", _fp), ("cst1", _fp), ("hT2", _fp), ("cst2", _fp), ("gx2", _fp), ("part", _fp), ("y", _fp),
                ("y_sb", _i64), ("y_st", _i64), ("y_su", _i64), ("y_sg", _i64),
                ("B", _i32), ("Bp", _i32), ("T", _i32), ("H", _i32), ("G", _i32), ("eps", _f32), ("slices", _i32), ("tc", _i32), ("lag", _i32),
                ("pad_", _i32), ("state_in", _fp), ("state_out", _fp)]


class GlstmpDesc(C.Structure):
    _fields_ = [("gx1", _fp), ("w1", _fp), ("w2i", _fp), ("w2h", _fp), ("r2", _fp), ("c2", _fp), ("gran", _fp), ("status", _fp),
                ("y", _fp), ("y_sb", _i64), ("y_st", _i64), ("y_su", _i64), ("y_sg", _i64),
                ("B", _i32), ("Bp", _i32), ("T", _i32), ("H", _i32), ("G", _i32), ("eps", _f32)]


class RowlnDesc(C.Structure):
    _fields_ = [("in_", _fp), ("gamma", _fp), ("beta", _fp), ("slope", _fp), ("out", _fp), ("out_sb", _i64),
                ("B", _i32), ("C", _i32), ("T", _i32), ("F", _i32), ("eps", _f32), ("pad_", _i32)]


class DenseDesc(C.Structure):
    _fields_ = [("D", _fp), ("w", _fp), ("bias", _fp), ("gamma", _fp), ("beta", _fp), ("slope", _fp),
                ("B", _i32), ("T", _i32), ("F", _i32), ("G", _i32), ("tpad", _i32), ("g_in", _i32), ("cin", _i32), ("g_out", _i32),
                ("dil", _i32), ("np", _i32), ("eps", _f32), ("wexp", _i32)]


class RowlnbDesc(C.Structure):
    _fields_ = [("in_", _fp), ("gamma", _fp), ("beta", _fp), ("slope", _fp), ("out", _fp),
                ("in_sb", _i64), ("in_sc", _i64), ("in_st", _i64), ("out_sb", _i64), ("out_sg", _i64), ("out_st", _i64),
                ("B", _i32), ("C", _i32), ("T", _i32), ("F", _i32), ("eps", _f32), ("pad_", _i32)]


class ChlnDesc(C.Structure):
    _fields_ = [("in_", _fp), ("gamma", _fp), ("beta", _fp), ("out", _fp), ("plane", _i64),
                ("B", _i32), ("C", _i32), ("eps", _f32), ("pad_", _i32)]


class AttnDesc(C.Structure):
    _fields_ = [("qkv", _fp), ("out", _fp), ("B", _i32), ("T", _i32), ("F", _i32), ("E", _i32),
                ("heads", _i32), ("axis", _i32), ("pad0_", _i32), ("pad1_", _i32), ("seqlen", _fp)]


class GruDesc(C.Structure):
    _fields_ = [("gx", _fp), ("whh", _fp), ("bhh", _fp), ("y", _fp),
                ("B", _i32), ("T", _i32), ("F", _i32), ("H", _i32), ("axis", _i32), ("split", _i32),
                ("x", _fp), ("wih", _fp), ("bih", _fp), ("seqlen", _fp)]


class GncombDesc(C.Structure):
    _fields_ = [("base", _fp), ("row", _fp), ("col", _fp), ("g_row", _fp), ("b_row", _fp), ("g_col", _fp),
                ("b_col", _fp), ("stats", _fp), ("out", _fp), ("plane", _i64), ("B", _i32), ("C", _i32),
                ("k1", _f32), ("k2", _f32), ("eps", _f32), ("pad_", _i32),
                ("frames", _fp), ("per_frame", _i32), ("pad1_", _i32)]


class AhamDesc(C.Structure):
    _fields_ = [("x", _fp * 4), ("w", _fp), ("means", _fp), ("out", _fp), ("plane", _i64),
                ("B", _i32), ("C", _i32), ("bias", _f32), ("pad_", _i32),
                ("frames", _fp), ("per_frame", _i32), ("pad1_", _i32)]


class QsampleDesc(C.Structure):
    _fields_ = [("label", _fp), ("init", _fp), ("noise", _fp), ("a", _fp), ("s", _fp), ("out", _fp),
                ("plane", _i64), ("B", _i32), ("mode", _i32)]


class MasklossDesc(C.Structure):
    _fields_ = [("esti", _fp), ("label", _fp), ("frames", _fp), ("partial", _fp), ("out", _fp),
                ("B", _i32), ("C", _i32), ("T", _i32), ("F", _i32)]


class TransposeDesc(C.Structure):
    _fields_ = [("in_", _fp), ("out", _fp), ("N", _i32), ("R", _i32), ("Cc", _i32), ("pad_", _i32)]


class TcmDesc(C.Structure):
    _fields_ = [("x", _fp), ("h", _fp), ("x_out", _fp), ("h_out", _fp), ("wbr", _fp), ("bmain", _fp), ("bmask", _fp),
                ("xf", _fp), ("wc2", _fp), ("bc2", _fp), ("xf2", _fp), ("wn1", _fp), ("bn1", _fp),
                ("slope_main", _f32), ("slope_mask", _f32), ("slope2", _f32), ("dil", _i32), ("B", _i32), ("T", _i32),
                ("frames", _fp)]


class Tcm2Desc(C.Structure):
    _fields_ = [("x", _fp), ("x_out", _fp), ("hs", _fp), ("hs_out", _fp), ("wbr", _fp), ("wc2", _fp), ("wn1", _fp),
                ("par", _fp), ("slope2", _f32), ("slope_main_next", _f32), ("slope_mask_next", _f32),
                ("dil", _i32), ("B", _i32), ("T", _i32), ("mode", _i32), ("np", _i32), ("qexp", _i32 * 3),
                ("frames", _fp)]


TCM2S_MAX = 20


class Tcm2sDesc(C.Structure):
    """The whole TCM stack as one launch (include/pdse.h: pdse_tcm2s_desc, csrc/tcm2.hip: tcm2s_kernel)."""
    _fields_ = [("blk", Tcm2Desc * TCM2S_MAX), ("flags", _fp), ("status", _fp), ("n", _i32), ("pad_", _i32)]


class BgluDesc(C.Structure):
    """BiConv(Trans)GLU block on plane tensors (include/pdse.h: pdse_bglu_desc, csrc/bglu.hip)."""
    _fields_ = [("hp", _fp), ("hp_sb", _i64), ("hp_Tp", _i32), ("hp_Fp", _i32), ("hp_t0", _i32), ("hp_f0", _i32),
                ("x0", Src), ("x1", Src), ("Tin", _i32), ("Fin", _i32), ("ntaps", _i32), ("sf_in", _i32),
                ("tap_dt", _i32 * 10), ("tap_df", _i32 * 10), ("p1mask", _i32), ("Fout1", _i32),
                ("B", _i32), ("Tout", _i32), ("Fout", _i32), ("np", _i32),
                ("w0", _fp), ("w1", _fp), ("w2", _fp), ("w3", _fp), ("wlc", _fp), ("wrc", _fp), ("wc2", _fp), ("wc2v", _fp),
                ("nx_w", _fp), ("bias0", _fp), ("bias1", _fp), ("bias0_t0", _fp), ("bias1_t0", _fp), ("bias_sb", _i64),
                ("blc", _fp), ("brc", _fp), ("bc2", _fp), ("slope", _f32), ("C2", _i32),
                ("out", _fp), ("out_sb", _i64), ("out_sc", _i64), ("out_st", _i64), ("out_sf", _i64), ("out_off", _i64),
                ("hp_par", _i32), ("nx_n", _i32),
                ("nx_hp", _fp), ("nx_hp_sb", _i64), ("nx_Tp", _i32), ("nx_Fp", _i32), ("nx_t0", _i32), ("nx_f0", _i32),
                ("nx_row0", _i32), ("nx_par", _i32),
                ("nx_add", _fp), ("add_sb", _i64), ("add_sc", _i64), ("add_st", _i64), ("add_sf", _i64),
                ("nx_out", _fp * 2), ("nx_sb", _i64 * 2), ("nx_sc", _i64 * 2), ("nx_st", _i64 * 2), ("nx_sf", _i64 * 2),
                ("nx_bias", _fp * 3), ("nx_bias_sb", _i64 * 3), ("skip_Fh", _i32), ("nx_items", _i32), ("qexp", _i32 * 4)]


class PlanesDesc(C.Structure):
    _fields_ = [("in_", _fp), ("in_sb", _i64), ("in_sc", _i64), ("in_st", _i64), ("in_sf", _i64),
                ("hp", _fp), ("hp_sb", _i64), ("hp_Tp", _i32), ("hp_Fp", _i32), ("hp_t0", _i32), ("hp_f0", _i32),
                ("B", _i32), ("T", _i32), ("F", _i32), ("np", _i32),
                ("in1", _fp), ("w", _fp * 2), ("bias", _fp * 2), ("bias_sb", _i64), ("hp1", _fp),
                ("cin0", _i32), ("cin1", _i32), ("nd", _i32), ("pad_", _i32)]


class CrmDesc(C.Structure):
    _fields_ = [("x", _fp), ("o", _fp), ("ri", _fp), ("out", _fp), ("a1", _f32), ("b1", _f32), ("a2", _f32), ("b2", _f32),
                ("a3", _f32), ("b3", _f32), ("plane", _i32), ("B", _i32), ("mode", _i32), ("pad_", _i32)]


class GcrnLastDesc(C.Structure):
    _fields_ = [("in0", _fp), ("in1", _fp), ("w1", _fp), ("w2", _fp), ("fcT", _fp), ("fcb", _fp), ("out", _fp),
                ("out_sb", _i64), ("b1", _f32), ("b2", _f32), ("bn_scale", _f32), ("bn_shift", _f32), ("B", _i32), ("T", _i32),
                ("fcp", _fp)]


class MetricsDesc(C.Structure):
    """Objective quality scores of B utterance pairs (include/pdse.h: pdse_metrics_desc, csrc/metrics.hip; with
    ``measures = METRICS_STOI`` also STOI and ESTOI, csrc/stoi.hip)."""
    _fields_ = [("clean", _fp), ("proc", _fp), ("lens_host", _fp), ("lens", _fp), ("tables", _fp), ("frames", _fp),
                ("sorted", _fp), ("out", _fp), ("B", _i32), ("Lmax", _i32), ("Mmax", _i32), ("measures", _i32),
                ("stoi_tables", _fp), ("stoi_work", _fp), ("stoi_out", _fp)]


class ResampleDesc(C.Structure):
    """PCM decode, mono mix and rate conversion of B utterances (include/pdse.h: pdse_resample_desc, csrc/resample.hip)."""
    _fields_ = [("pcm", _fp), ("offs", _fp), ("n_in_host", _fp), ("n_in", _fp), ("taps", _fp), ("out", _fp),
                ("pcm_bytes", _i64), ("B", _i32), ("Lmax", _i32), ("up", _i32), ("down", _i32), ("half", _i32),
                ("width", _i32), ("ch", _i32), ("fmt", _i32)]


class RangeRow(C.Structure):
    """One tensor of a range audit (include/pdse.h: pdse_range_row)."""
    _fields_ = [("ptr", _fp), ("n", _i64), ("s0", _i64), ("s1", _i64), ("s2", _i64),
                ("n0", _i32), ("n1", _i32), ("n2", _i32), ("n3", _i32), ("i0", _i32), ("par_half", _i32),
                ("kind", _i32), ("exp", _i32), ("out_row", _i32), ("pad_", _i32)]


class RangeDesc(C.Structure):
    """Binade histograms of a table of tensors (include/pdse.h: pdse_range_desc, csrc/range.hip)."""
    _fields_ = [("rows", _fp), ("out", _fp),
                ("nrows", _i32), ("out_rows", _i32), ("mode", _i32), ("blocks", _i32)]


RANGE_BINS = 32            # PDSE_RANGE_BINS
RANGE_F32, RANGE_F16HI = 0, 1
RANGE_CLEAR, RANGE_ACCUMULATE = 0, 1
RANGE_NONFINITE = 2        # PDSE_RANGE_NONFINITE: out[r][0] += Inf / NaN elements of the fp32 tensor of row r
# The bin map of csrc/range.hip, decided there once: RANGE_BINADE[bin] is the exponent E of the bin's lower edge 2^E in scaled
# units.  Bin 0 counts zeros (None); bin 1 everything non-zero below 2^-14 (-inf: hi is an fp16 subnormal); bins 2 .. 30 one
# normal fp16 binade each, E = -14 .. 14; bin 31 starts at 2^15 and also takes infinities and NaN.
RANGE_BINADE = (None, float("-inf")) + tuple(range(-14, 15)) + (15,)
RANGE_BIN_FULL = RANGE_BINADE.index(-2)      # first bin whose elements are carried at full precision (lo a normal fp16)
RANGE_BIN_TOP = RANGE_BINS - 1               # hi leaves the fp16 range

RESAMPLE_BLOCK = 256      # PDSE_RESAMPLE_BLOCK: outputs per workgroup
# pdse_resample_desc.fmt: 0 is the integer-PCM operator as it was (width 1 / 2 / 4, one or two channels); the others (PDSE_WAV_*)
WAV_INT, WAV_FLOAT, WAV_ALAW, WAV_ULAW = 1, 2, 3, 4
WAV_SPLIT = 256           # PDSE_WAV_SPLIT: OR-ed onto WAV_INT .. WAV_ULAW, the channels kept apart (out [B ch][Lmax])
WAV_MAX_CH = 8            # PDSE_WAV_MAX_CH: channels the kernel of fmt != 0 mixes
WAVOUT_IMAGE_BYTES = RESAMPLE_BLOCK * WAV_MAX_CH * 4 + 16     # csrc/wavout.hip: LDS image of a block's bytes, beside its input window
WAVCH_STATIC_BYTES = WAVOUT_IMAGE_BYTES + 256                 # csrc/wavout.hip: static LDS of the channel encoder, beside its ch windows

METRICS_OFF_WIN, METRICS_OFF_BASIS = 0, 512
METRICS_OFF_CRIT = METRICS_OFF_BASIS + 480 * 1024
METRICS_OFF_WEPS = METRICS_OFF_CRIT + 25 * 512
METRICS_OFF_BRANGE = METRICS_OFF_WEPS + 2 * 512
METRICS_TABLE_DOUBLES = METRICS_OFF_BRANGE + 64

METRICS_STOI = 1          # PDSE_METRICS_STOI: pdse_metrics_desc.measures
STOI_OFF_WIN, STOI_OFF_BASIS = 0, 256
STOI_OFF_BRANGE = STOI_OFF_BASIS + 256 * 512
STOI_OFF_TAPS = STOI_OFF_BRANGE + 32
STOI_TABLE_DOUBLES = STOI_OFF_TAPS + 264


def stoi_n10(length):
    """PDSE_STOI_N10: samples at 10 kHz of ``length`` samples at 16 kHz."""
    return (int(length) * 5 + 7) // 8


def stoi_frames(length):
    """PDSE_STOI_FRAMES: whole 256-sample frames every 128 of those samples."""
    n = stoi_n10(length)
    return 0 if n < 256 else 1 + (n - 256) // 128


def stoi_work_doubles(B, Lmax):
    """PDSE_STOI_WORK_DOUBLES: float64 elements of pdse_metrics_desc.stoi_work."""
    F = stoi_frames(Lmax)
    return int(B) * (stoi_n10(Lmax) + F + (F + 3) // 2 + 30 * F)

# The operator table, in kind order: (kind, descriptor mirror, direct entry of include/pdse.h).  Everything below that exists
# once per operator is derived from it; tests/test_abi.py holds every row, and every mirror's layout, against the header.
OPS = (
    (OP_GCONV, GconvDesc, "pdse_gconv_f32"),
    (OP_TIME, TimeDesc, "pdse_time_embed_f32"),
    (OP_EW, EwDesc, "pdse_ew_f32"),
    (OP_COMPAND, CompandDesc, "pdse_compand_f32"),
    (OP_WAVPREP, WavprepDesc, "pdse_wavprep_f32"),
    (OP_OLA, OlaDesc, "pdse_ola_f32"),
    (OP_SIGMA, SigmaDesc, "pdse_sigma_mask_f32"),
    (OP_LN, LnDesc, "pdse_layernorm_f32"),
    (OP_LSTM, LstmDesc, "pdse_lstm_f32"),
    (OP_ROWLN, RowlnDesc, "pdse_rowln_prelu_f32"),
    (OP_CHLN, ChlnDesc, "pdse_chln_f32"),
    (OP_ATTN, AttnDesc, "pdse_attention_f32"),
    (OP_GRU, GruDesc, "pdse_bigru_f32"),
    (OP_GNCOMB, GncombDesc, "pdse_gn_combine_f32"),
    (OP_AHAM, AhamDesc, "pdse_aham_f32"),
    (OP_QSAMPLE, QsampleDesc, "pdse_qsample_f32"),
    (OP_TRANSPOSE, TransposeDesc, "pdse_transpose_f32"),
    (OP_TCM, TcmDesc, "pdse_tcm_f32"),
    (OP_CRM, CrmDesc, "pdse_crm_f32"),
    (OP_GCRNLAST, GcrnLastDesc, "pdse_gcrnlast_f32"),
    (OP_MASKLOSS, MasklossDesc, "pdse_masked_mse_f32"),
    (OP_GLSTM, GlstmDesc, "pdse_glstm_f32"),
    (OP_TCM2, Tcm2Desc, "pdse_tcm2_bf16x3"),
    (OP_BGLU, BgluDesc, "pdse_bglu_planes"),
    (OP_PLANES, PlanesDesc, "pdse_split_planes"),
    (OP_GLSTMP, GlstmpDesc, "pdse_glstm_persistent_f32"),
    (OP_TCM2S, Tcm2sDesc, "pdse_tcm2_stack_bf16x3"),
    (OP_DENSE, DenseDesc, "pdse_dense_layer_bf16x3"),
    (OP_ROWLNB, RowlnbDesc, "pdse_rowln_blocked_f32"),
    (OP_METRICS, MetricsDesc, "pdse_quality_metrics_f32"),
    (OP_RESAMPLE, ResampleDesc, "pdse_pcm_resample_f32"),
    (OP_RANGE, RangeDesc, "pdse_range_hist"),
)
DESC_TYPES = {kind: typ for kind, typ, _ in OPS}
KIND_OF = {typ: kind for kind, typ, _ in OPS}
_DIRECT = {kind: name for kind, _, name in OPS}

EXPORTS = [
    "pdse_abi_version", "pdse_last_error", "pdse_desc_size", "pdse_bglu_set_form",
    "pdse_plan_create", "pdse_plan_add", "pdse_plan_size", "pdse_plan_set_device", "pdse_plan_clear", "pdse_plan_run",
    "pdse_plan_run_range",
    "pdse_plan_build_graph", "pdse_plan_launch_graph", "pdse_plan_time_ops", "pdse_plan_time_tag",
    "pdse_plan_destroy", "pdse_plan_load", "pdse_plan_region", "pdse_prior_forward", "pdse_eps_forward", "pdse_enhance",
    "pdse_wav_encode", "pdse_wav_encode_channels", "pdse_pair_prep", "pdse_spec_losses", "pdse_spec_frames",
    "pdse_spec_frames_mode",
    "pdse_objective_noise", "pdse_sigma_loss", "pdse_ensemble_stats", "pdse_window_gather", "pdse_window_scatter",
] + [name for _, _, name in OPS]


class PdseError(RuntimeError):
    """Non-zero status from libpdse.so (the reference raises Python exceptions only)."""


class PdseRangeError(PdseError):
    """A pass on f16x2 operands left the fp16 window of include/pdse.h (PDSE_F16_ACT_EXP): an activation went beyond its top
    (its planes became infinities: non-finite output), or - seen by the range audit only, ``SamplerPipeline(audit=True)`` -
    a whole tensor stayed below its bottom, where no element keeps a normal lo part.  The same pass on the three-plane bf16
    split has no such window."""


_lib = None


def load():
    """Load libpdse.so once; verify ABI version and descriptor sizes."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64 (soname libamdhip64.so.7, the soname libpdse.so needs):
    # it must be in the process first so that both share ONE HIP/HSA runtime — two runtimes
    # in one process lose the device ("no ROCm-capable device is detected").
    import torch  # noqa: F401

    if not os.path.exists(LIB_PATH):
        raise PdseError(
            "libpdse.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " (hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise PdseError("libpdse.so lacks symbol %s declared in include/pdse.h" % name)
    lib.pdse_last_error.restype = C.c_char_p
    lib.pdse_abi_version.restype = C.c_int
    lib.pdse_desc_size.argtypes = [C.c_int]
    for kind, name in _DIRECT.items():
        getattr(lib, name).argtypes = [C.POINTER(DESC_TYPES[kind]), C.c_void_p]
        getattr(lib, name).restype = C.c_int
    lib.pdse_plan_create.argtypes = [C.POINTER(C.c_void_p)]
    lib.pdse_plan_add.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.pdse_plan_size.argtypes = [C.c_void_p]
    lib.pdse_plan_set_device.argtypes = [C.c_void_p, C.c_int]
    lib.pdse_plan_clear.argtypes = [C.c_void_p]
    lib.pdse_plan_run.argtypes = [C.c_void_p, C.c_void_p]
    lib.pdse_plan_run_range.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.pdse_plan_build_graph.argtypes = [C.c_void_p, C.c_void_p]
    lib.pdse_plan_launch_graph.argtypes = [C.c_void_p, C.c_void_p]
    lib.pdse_plan_time_ops.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]
    lib.pdse_plan_time_tag.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float),
                                       C.POINTER(C.c_int)]
    lib.pdse_plan_destroy.argtypes = [C.c_void_p]
    lib.pdse_plan_destroy.restype = None
    lib.pdse_wav_encode.argtypes = [_fp] * 8 + [_i64] + [_i32] * 8 + [C.c_void_p]
    lib.pdse_wav_encode.restype = C.c_int
    lib.pdse_wav_encode_channels.argtypes = lib.pdse_wav_encode.argtypes
    lib.pdse_wav_encode_channels.restype = C.c_int
    lib.pdse_pair_prep.argtypes = [_fp] * 6 + [_i32] * 4 + [C.c_void_p]
    lib.pdse_pair_prep.restype = C.c_int
    lib.pdse_spec_losses.argtypes = [_fp] * 7 + [_i32] * 3 + [C.c_void_p]
    lib.pdse_spec_losses.restype = C.c_int
    lib.pdse_spec_frames.argtypes = [_fp] * 3 + [_i32] * 3 + [C.c_void_p]
    lib.pdse_spec_frames.restype = C.c_int
    lib.pdse_spec_frames_mode.argtypes = [_fp] * 3 + [_i32] * 4 + [C.c_void_p]
    lib.pdse_spec_frames_mode.restype = C.c_int
    lib.pdse_objective_noise.argtypes = [_fp] * 9 + [_i32] * 5 + [C.c_void_p]
    lib.pdse_objective_noise.restype = C.c_int
    lib.pdse_sigma_loss.argtypes = [_fp] * 9 + [_i32] * 3 + [C.c_void_p]
    lib.pdse_sigma_loss.restype = C.c_int
    lib.pdse_ensemble_stats.argtypes = [_fp] * 8 + [_i32] * 4 + [C.c_void_p]
    lib.pdse_ensemble_stats.restype = C.c_int
    lib.pdse_window_gather.argtypes = [_fp] * 2 + [_i32] * 6 + [C.c_void_p]
    lib.pdse_window_gather.restype = C.c_int
    lib.pdse_window_scatter.argtypes = [_fp] * 2 + [_i32] * 8 + [C.c_void_p]
    lib.pdse_window_scatter.restype = C.c_int
    if lib.pdse_abi_version() != ABI_VERSION:
        raise PdseError("libpdse.so ABI %d != binding ABI %d" % (lib.pdse_abi_version(), ABI_VERSION))
    for kind, typ in DESC_TYPES.items():
        if lib.pdse_desc_size(kind) != C.sizeof(typ):
            raise PdseError("descriptor %s: library sizeof %d != binding sizeof %d"
                            % (typ.__name__, lib.pdse_desc_size(kind), C.sizeof(typ)))
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        raise PdseError("%s failed: %s" % (what or "libpdse call", load().pdse_last_error().decode()))


def launch(desc, stream=0, device=None):
    """Launch one operator directly (on ``device`` when given, else on the current device)."""
    lib = load()
    name = _DIRECT[KIND_OF[type(desc)]]
    on = contextlib.nullcontext()
    if device is not None:
        import torch

        on = torch.cuda.device(device)
    with on:
        check(getattr(lib, name)(C.byref(desc), C.c_void_p(stream)), name)


def wav_encode(x, n_in_host, n_keep_host, n_in, n_keep, taps, out, clipped, stride, B, Lmax, up, down, half, fmt, width, ch,
               stream=0, device=None, entry="pdse_wav_encode"):
    """pdse_wav_encode (include/pdse.h: the wav back end, csrc/wavout.hip): pointers as integers, plain arguments."""
    lib = load()
    on = contextlib.nullcontext()
    if device is not None:
        import torch

        on = torch.cuda.device(device)
    with on:
        check(getattr(lib, entry)(x, n_in_host, n_keep_host, n_in, n_keep, taps, out, clipped, int(stride), int(B), int(Lmax),
                                  int(up), int(down), int(half), int(fmt), int(width), int(ch), C.c_void_p(stream)), entry)


def wav_encode_channels(*args, **kw):
    """pdse_wav_encode_channels (include/pdse.h: the channel encoder): ``wav_encode``'s arguments with x [B ch][Lmax] and
    clipped [B][blocks][ch]."""
    wav_encode(*args, entry="pdse_wav_encode_channels", **kw)


def _on(device):
    if device is None:
        return contextlib.nullcontext()
    import torch

    return torch.cuda.device(device)


def pair_prep(noisy, clean, lens, noisy_pad, clean_pad, c, B, L, pad=160, reflect_own=0, stream=0, device=None):
    """pdse_pair_prep (include/pdse.h: the pair front end of the validation epoch, csrc/valid.hip): pointers as integers."""
    lib = load()
    with _on(device):
        check(lib.pdse_pair_prep(noisy, clean, lens, noisy_pad, clean_pad, c, int(B), int(L), int(pad), int(reflect_own),
                                 C.c_void_p(stream)), "pdse_pair_prep")


def spec_losses(esti, label, frames_host, frames, partial, per_utt, loss, B, T, F, stream=0, device=None):
    """pdse_spec_losses (include/pdse.h: the masked losses of the validation epoch, csrc/valid.hip): pointers as integers."""
    lib = load()
    with _on(device):
        check(lib.pdse_spec_losses(esti, label, frames_host, frames, partial, per_utt, loss, int(B), int(T), int(F),
                                   C.c_void_p(stream)), "pdse_spec_losses")


def spec_frames(spec, basis, frames, B, T, F, stream=0, device=None):
    """pdse_spec_frames (include/pdse.h: decompression and inverse DFT in double for the scored waveforms, csrc/valid.hip)."""
    lib = load()
    with _on(device):
        check(lib.pdse_spec_frames(spec, basis, frames, int(B), int(T), int(F), C.c_void_p(stream)), "pdse_spec_frames")


def spec_frames_mode(spec, basis, frames, B, T, F, mode, stream=0, device=None):
    """pdse_spec_frames_mode (include/pdse.h: pdse_spec_frames with the decompress mode of a feat_type, csrc/valid.hip)."""
    lib = load()
    with _on(device):
        check(lib.pdse_spec_frames_mode(spec, basis, frames, int(B), int(T), int(F), int(mode), C.c_void_p(stream)),
              "pdse_spec_frames_mode")


def objective_noise(label, init, noise, t, a_tab, s_tab, noisy, target, maxbuf, B, T, F, mode=0, sigma=0, stream=0, device=None):
    """pdse_objective_noise (include/pdse.h: the forward noising of the denoising objective, csrc/objective.hip): pointers as integers."""
    lib = load()
    with _on(device):
        check(lib.pdse_objective_noise(label, init, noise, t, a_tab, s_tab, noisy, target, maxbuf, int(B), int(T), int(F), int(mode),
                                       int(sigma), C.c_void_p(stream)), "pdse_objective_noise")


def sigma_loss(predicted, target, init, maxbuf, frames_host, frames, partial, per_utt, loss, B, T, F, stream=0, device=None):
    """pdse_sigma_loss (include/pdse.h: com_mse_sigma_loss of the denoising objective, csrc/objective.hip): pointers as integers."""
    lib = load()
    with _on(device):
        check(lib.pdse_sigma_loss(predicted, target, init, maxbuf, frames_host, frames, partial, per_utt, loss, int(B), int(T), int(F),
                                  C.c_void_p(stream)), "pdse_sigma_loss")


def ensemble_stats(members, mean, spread, frames_host, frames, partial, per_utt, per_member, K, B, T, F, stream=0, device=None):
    """pdse_ensemble_stats (include/pdse.h: mean, spread and sums of a member-major ensemble, csrc/ensemble.hip): pointers as integers."""
    lib = load()
    with _on(device):
        check(lib.pdse_ensemble_stats(members, mean, spread, frames_host, frames, partial, per_utt, per_member, int(K), int(B), int(T),
                                      int(F), C.c_void_p(stream)), "pdse_ensemble_stats")


def window_gather(whole, win, B, C_, T, F, W, a, stream=0, device=None):
    """pdse_window_gather (include/pdse.h: frames [a, a + W) of a whole-file tensor into a window, csrc/window.hip): pointers as integers."""
    lib = load()
    with _on(device):
        check(lib.pdse_window_gather(whole, win, int(B), int(C_), int(T), int(F), int(W), int(a), C.c_void_p(stream)), "pdse_window_gather")


def window_scatter(win, whole, B, C_, T, F, W, a, keep_lo, keep_hi, stream=0, device=None):
    """pdse_window_scatter (include/pdse.h: a window's kept frames back to their whole-file position, csrc/window.hip)."""
    lib = load()
    with _on(device):
        check(lib.pdse_window_scatter(win, whole, int(B), int(C_), int(T), int(F), int(W), int(a), int(keep_lo), int(keep_hi),
                                      C.c_void_p(stream)), "pdse_window_scatter")


class Plan:
    """Recorded operator sequence replayed by one C call (include/pdse.h, plans)."""

    def __init__(self, device=None):
        """device: torch device (or ordinal) the plan's buffers live on; every run makes it current for the call."""
        self._lib = load()
        h = C.c_void_p()
        check(self._lib.pdse_plan_create(C.byref(h)), "pdse_plan_create")
        self._h = h
        if device is not None:
            import torch

            dev = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
            idx = dev.index if dev.index is not None else torch.cuda.current_device()
            check(self._lib.pdse_plan_set_device(self._h, int(idx)), "pdse_plan_set_device")
        self._keep = []  # python-side owners of every buffer named by a descriptor
        self.has_graph = False

    def add(self, desc, tag=0, keep=()):
        check(self._lib.pdse_plan_add(self._h, KIND_OF[type(desc)], C.byref(desc), int(tag)), "pdse_plan_add")
        self._keep.extend(keep)
        return len(self) - 1

    def keep(self, *objs):
        self._keep.extend(objs)

    def __len__(self):
        return self._lib.pdse_plan_size(self._h)

    def run(self, stream=0):
        check(self._lib.pdse_plan_run(self._h, C.c_void_p(stream)), "pdse_plan_run")

    def run_range(self, begin, end, stream=0):
        check(self._lib.pdse_plan_run_range(self._h, begin, end, C.c_void_p(stream)), "pdse_plan_run_range")

    def build_graph(self, stream):
        check(self._lib.pdse_plan_build_graph(self._h, C.c_void_p(stream)), "pdse_plan_build_graph")
        self.has_graph = True

    def launch_graph(self, stream):
        check(self._lib.pdse_plan_launch_graph(self._h, C.c_void_p(stream)), "pdse_plan_launch_graph")

    def time_ops(self, begin, end, stream=0):
        buf = (C.c_float * (end - begin))()
        check(self._lib.pdse_plan_time_ops(self._h, begin, end, C.c_void_p(stream), buf), "pdse_plan_time_ops")
        return list(buf)

    def time_tag(self, tag, stream=0):
        ms, cnt = C.c_float(), C.c_int()
        check(self._lib.pdse_plan_time_tag(self._h, tag, C.c_void_p(stream), C.byref(ms), C.byref(cnt)),
              "pdse_plan_time_tag")
        return ms.value, cnt.value

    def __del__(self):
        try:
            if self._h:
                self._lib.pdse_plan_destroy(self._h)
                self._h = None
        except Exception:
            pass
