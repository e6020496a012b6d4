// internal helpers shared by the translation units of libpdse.so (not part of the ABI)
#ifndef PDSE_INTERNAL_H
#define PDSE_INTERNAL_H
#include <hip/hip_runtime.h>

#include "pdse.h"

void pdse_set_error(const char* msg);
// returns 0 when the last launch was accepted, else records "<what>: <hip error>" and returns 1
int pdse_check_launch(const char* what);
int pdse_check_hip(hipError_t e, const char* what);
// hipFuncAttributeMaxDynamicSharedMemorySize, once per (function, device): a plan may be bound to any device of the
// process (pdse_plan_set_device), and the attribute belongs to the device the function is loaded on.  `mask` is the
// caller's per-function record (bit d: done on device d).  Returns 0 on success.
int pdse_lds_attr(const void* fn, unsigned long long* mask, const char* what);
// Diagnostic hooks (clock-stamp traces, stage masks) exist only in -DPDSE_DIAG builds: in the product library the
// environment cannot change a launch (a stage mask gives wrong results; a trace mallocs / synchronises inside a launch,
// which is illegal during hipGraph capture).
#ifdef PDSE_DIAG
#define PDSE_DIAG_ENV(name) (getenv(name))
#else
#define PDSE_DIAG_ENV(name) ((const char*)nullptr)
#endif

// The operator table: one row X(KIND, stem, entry) per operator kind, in enumerator order.  A row names PDSE_OP_<KIND>, the
// descriptor pdse_<stem>_desc, its launcher pdse_<stem>_launch (and the member <stem> of a plan's descriptor union), and the
// public name of the direct launch, the one irregular part.  Everything that exists once per operator is generated from it:
// the launcher prototypes below, and in capi.hip the union, the size and launch switches and the direct entries, with a
// static_assert per row that it sits at its enumerator's index.  include/pdse.h, the ABI document, stays written out.
#define PDSE_OPS(X)                                                                            \
  X(GCONV, gconv, pdse_gconv_f32)                                                              \
  X(TIME, time, pdse_time_embed_f32)                                                           \
  X(EW, ew, pdse_ew_f32)                                                                       \
  X(COMPAND, compand, pdse_compand_f32)                                                        \
  X(WAVPREP, wavprep, pdse_wavprep_f32)                                                        \
  X(OLA, ola, pdse_ola_f32)                                                                    \
  X(SIGMA, sigma, pdse_sigma_mask_f32)                                                         \
  X(LN, ln, pdse_layernorm_f32)                                                                \
  X(LSTM, lstm, pdse_lstm_f32)                                                                 \
  X(ROWLN, rowln, pdse_rowln_prelu_f32)                                                        \
  X(CHLN, chln, pdse_chln_f32)                                                                 \
  X(ATTN, attn, pdse_attention_f32)                                                            \
  X(GRU, gru, pdse_bigru_f32)                                                                  \
  X(GNCOMB, gncomb, pdse_gn_combine_f32)                                                       \
  X(AHAM, aham, pdse_aham_f32)                                                                 \
  X(QSAMPLE, qsample, pdse_qsample_f32)                                                        \
  X(TRANSPOSE, transpose, pdse_transpose_f32)                                                  \
  X(TCM, tcm, pdse_tcm_f32)                                                                    \
  X(CRM, crm, pdse_crm_f32)                                                                    \
  X(GCRNLAST, gcrnlast, pdse_gcrnlast_f32)                                                     \
  X(MASKLOSS, maskloss, pdse_masked_mse_f32)                                                   \
  X(GLSTM, glstm, pdse_glstm_f32)                                                              \
  X(TCM2, tcm2, pdse_tcm2_bf16x3)                                                              \
  X(BGLU, bglu, pdse_bglu_planes)                                                              \
  X(PLANES, planes, pdse_split_planes)                                                         \
  X(GLSTMP, glstmp, pdse_glstm_persistent_f32)   /* csrc/lstmp.hip */                          \
  X(TCM2S, tcm2s, pdse_tcm2_stack_bf16x3)   /* csrc/tcm2.hip: the whole stack as one launch */ \
  X(DENSE, dense, pdse_dense_layer_bf16x3)   /* csrc/dense.hip */                              \
  X(ROWLNB, rowlnb, pdse_rowln_blocked_f32)                                                    \
  X(METRICS, metrics, pdse_quality_metrics_f32)   /* csrc/metrics.hip */                       \
  X(RESAMPLE, resample, pdse_pcm_resample_f32)   /* csrc/resample.hip */                       \
  X(RANGE, range, pdse_range_hist)   /* csrc/range.hip */

#define X(KIND, stem, entry) int pdse_##stem##_launch(const pdse_##stem##_desc* d, hipStream_t s);
PDSE_OPS(X)
#undef X
int pdse_gconv2_launch(const pdse_gconv_desc* d, hipStream_t s);  // korder 1, validated by pdse_gconv_launch
int pdse_gconv3_launch(const pdse_gconv_desc* d, hipStream_t s);  // korder 2 (split-bf16 BIGLU), validated there too
int pdse_gconv4_launch(const pdse_gconv_desc* d, hipStream_t s);  // korder 3 (split-bf16 GEMM-shaped LINEAR / GLU)
// korder 5 GLU: the even (d) and odd (e) output bins of a transposed convolution as one launch (pdse.h: p1mask with w2 == NULL).
// A plan checks the pair when e is added (capi.hip) and launches it unchecked afterwards.
int pdse_gconv_pair_check(const pdse_gconv_desc* d, const pdse_gconv_desc* e);     // both descriptors, then:
int pdse_gconv4_pair_check(const pdse_gconv_desc* d, const pdse_gconv_desc* e);    // that e is d's odd phase
int pdse_gconv4_pair_launch(const pdse_gconv_desc* d, const pdse_gconv_desc* e, hipStream_t s);
int pdse_stoi_launch(const pdse_metrics_desc* d, hipStream_t s);   /* csrc/stoi.hip, reached through pdse_metrics_launch (measures) */
int pdse_gru3_launch(const pdse_gru_desc* d, hipStream_t s);   /* csrc/gru3.hip, reached through pdse_gru_launch */
// csrc/wavout.hip: the wav back end behind pdse_wav_encode (plain arguments: no descriptor, no operator kind, not recordable in a plan)
int pdse_wavout_launch(const float* x, const int32_t* n_in_host, const int32_t* n_keep_host, const int32_t* n_in, const int32_t* n_keep,
                       const double* taps, uint8_t* out, int32_t* clipped, int64_t stride, int32_t B, int32_t Lmax, int32_t up,
                       int32_t down, int32_t half, int32_t fmt, int32_t width, int32_t ch, hipStream_t s);
// csrc/wavout.hip: the channel encoder behind pdse_wav_encode_channels (x [B ch][Lmax], clipped [B][blocks][ch]; plain arguments too)
int pdse_wavch_launch(const float* x, const int32_t* n_in_host, const int32_t* n_keep_host, const int32_t* n_in, const int32_t* n_keep,
                      const double* taps, uint8_t* out, int32_t* clipped, int64_t stride, int32_t B, int32_t Lmax, int32_t up,
                      int32_t down, int32_t half, int32_t fmt, int32_t width, int32_t ch, hipStream_t s);
// csrc/valid.hip: the pair front end and the masked losses of the validation epoch behind pdse_pair_prep / pdse_spec_losses (plain arguments too)
int pdse_pair_prep_launch(const float* noisy, const float* clean, const int32_t* lens, float* noisy_pad, float* clean_pad, float* c,
                          int32_t B, int32_t L, int32_t pad, int32_t reflect_own, hipStream_t s);
int pdse_spec_losses_launch(const float* esti, const float* label, const int32_t* frames_host, const int32_t* frames, double* partial,
                            double* per_utt, float* loss, int32_t B, int32_t T, int32_t F, hipStream_t s);
int pdse_spec_frames_launch(const float* spec, const double* basis, float* frames, int32_t B, int32_t T, int32_t F, hipStream_t s);
int pdse_spec_frames_mode_launch(const float* spec, const double* basis, float* frames, int32_t B, int32_t T, int32_t F, int32_t mode,
                                 hipStream_t s);
// csrc/objective.hip: the forward noising and the --sigma loss of the denoising objective behind pdse_objective_noise / pdse_sigma_loss (plain arguments too)
int pdse_objective_noise_launch(const float* label, const float* init, const float* noise, const int32_t* t, const float* a_tab,
                                const float* s_tab, float* noisy, float* target, float* maxbuf, int32_t B, int32_t T, int32_t F,
                                int32_t mode, int32_t sigma, hipStream_t s);
int pdse_sigma_loss_launch(const float* predicted, const float* target, const float* init, const float* maxbuf,
                           const int32_t* frames_host, const int32_t* frames, double* partial, double* per_utt, float* loss, int32_t B,
                           int32_t T, int32_t F, hipStream_t s);
// csrc/ensemble.hip: the statistics of a posterior ensemble behind pdse_ensemble_stats (plain arguments too)
int pdse_ensemble_stats_launch(const float* members, float* mean, float* spread, const int32_t* frames_host, const int32_t* frames,
                               double* partial, double* per_utt, double* per_member, int32_t K, int32_t B, int32_t T, int32_t F,
                               hipStream_t s);
// csrc/window.hip: gather / scatter of the windowed passes behind pdse_window_gather / pdse_window_scatter (plain arguments too)
int pdse_window_gather_launch(const float* whole, float* win, int32_t B, int32_t C, int32_t T, int32_t F, int32_t W, int32_t a,
                              hipStream_t s);
int pdse_window_scatter_launch(const float* win, float* whole, int32_t B, int32_t C, int32_t T, int32_t F, int32_t W, int32_t a,
                               int32_t keep_lo, int32_t keep_hi, hipStream_t s);
int pdse_range_validate(const pdse_range_desc* d);               /* reads the row table back and checks it (direct launches, plan_add) */
#endif
