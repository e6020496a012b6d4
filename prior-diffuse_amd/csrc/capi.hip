// capi.hip — the extern "C" surface of libpdse.so (include/pdse.h): argument checks,
// per-thread error text, direct launches and recorded plans (replayable, graph-capturable).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "pdse.h"
#include "pdse_internal.h"

static thread_local std::string g_err;

void pdse_set_error(const char* msg) { g_err = msg ? msg : "unknown error"; }

int pdse_check_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return 0;
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return 1;
}

int pdse_check_launch(const char* what) { return pdse_check_hip(hipGetLastError(), what); }

int pdse_lds_attr(const void* fn, unsigned long long* mask, const char* what) {
  int dev = 0;
  if (pdse_check_hip(hipGetDevice(&dev), what)) return 1;
  if (dev >= 0 && dev < 64 && ((*mask >> dev) & 1ull)) return 0;
  if (pdse_check_hip(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), what)) return 1;
  if (dev >= 0 && dev < 64) *mask |= 1ull << dev;
  return 0;
}

#define X(KIND, stem, entry) pdse_##stem##_desc stem;
union pdse_any_desc {
  PDSE_OPS(X)
};
#undef X

// a row of PDSE_OPS in the wrong place, or a missing one, does not compile
#define X(KIND, stem, entry) ROW_##KIND,
enum { PDSE_OPS(X) ROW_COUNT };
#undef X
#define X(KIND, stem, entry) static_assert((int)ROW_##KIND == (int)PDSE_OP_##KIND, "PDSE_OPS: the row of " #KIND " is not at its enumerator's index");
PDSE_OPS(X)
#undef X
static_assert(ROW_COUNT == 32, "PDSE_OPS: one row per operator kind of include/pdse.h");

struct pdse_op {
  int kind;
  int tag;
  pdse_any_desc d;
};

// a device allocation owned by a plan that was loaded from a file (pdse_plan_load)
struct pdse_region {
  std::string name;      // empty: internal; else the name an input / output is found by (pdse_plan_region)
  void* ptr = nullptr;
  uint64_t bytes = 0;
};

struct pdse_plan {
  std::vector<pdse_op> ops;
  std::vector<pdse_region> regions;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  int device = -1;   // -1: whatever device is current on the calling thread
};

// Makes the plan's device current for the duration of a call and restores the caller's afterwards: every buffer of a
// plan lives on one device, and a stream handle of device N used while device 0 is current fails (or worse, launches on
// the wrong device).  One process per GPU with LOCAL_RANK != 0 is the case that needs it.
struct device_guard {
  int prev = -1;
  bool ok = true;
  explicit device_guard(const pdse_plan* p) {
    if (!p || p->device < 0) return;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != p->device) ok = !pdse_check_hip(hipSetDevice(p->device), "set device");
    else prev = -1;
  }
  ~device_guard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

static int op_size(int kind) {
  switch (kind) {
#define X(KIND, stem, entry) case PDSE_OP_##KIND: return (int)sizeof(pdse_##stem##_desc);
    PDSE_OPS(X)
#undef X
    default: return -1;
  }
}

static int launch_op(const pdse_op& op, hipStream_t s) {
  switch (op.kind) {
#define X(KIND, stem, entry) case PDSE_OP_##KIND: return pdse_##stem##_launch(&op.d.stem, s);
    PDSE_OPS(X)
#undef X
    default: pdse_set_error("plan: unknown op kind"); return 1;
  }
}

// A korder 5 GLU convolution whose descriptor names the next operator as its odd phase (pdse.h: p1mask with w2 == NULL).
static bool names_odd_phase(const pdse_op& op) {
  return op.kind == PDSE_OP_GCONV && op.d.gconv.korder == 5 && op.d.gconv.p1mask != 0 && op.d.gconv.w2 == nullptr;
}

// The operator about to follow the plan's last one: behind a descriptor that names its odd phase comes that phase and nothing
// else, checked here, once (pdse_plan_add, pdse_plan_load), so that a run is launches only.
static int check_follows(const pdse_plan* p, const pdse_op& op) {
  if (p->ops.empty() || !names_odd_phase(p->ops.back())) return 0;
  if (op.kind != PDSE_OP_GCONV) {
    pdse_set_error("plan: the operator behind a gconv that names its odd phase (p1mask, korder 5) must be that phase");
    return 1;
  }
  return pdse_gconv_pair_check(&p->ops.back().d.gconv, &op.d.gconv);
}

// Such a pair runs as one launch (csrc/gconv4.hip) when both operators lie in the range being run; *n: operators consumed.
static int launch_at(const pdse_plan* p, const int i, const int end, hipStream_t s, int* n) {
  const pdse_op& op = p->ops[i];
  *n = 1;
  if (names_odd_phase(op) && i + 1 < end) {
    *n = 2;
    return pdse_gconv4_pair_launch(&op.d.gconv, &p->ops[i + 1].d.gconv, s);
  }
  return launch_op(op, s);
}

// What a direct launch checks before the launcher's own argument checks: nothing, except for the range audit, whose row
// table is device data (pdse_plan_add checks it at add time instead, so that a plan run is launches only).
template <typename D>
static int validate_desc(const D*) { return 0; }
static int validate_desc(const pdse_range_desc* d) { return pdse_range_validate(d); }

extern "C" {

int pdse_abi_version(void) { return PDSE_ABI_VERSION; }
const char* pdse_last_error(void) { return g_err.c_str(); }
int pdse_desc_size(int op_kind) { return op_size(op_kind); }

#define X(KIND, stem, entry) \
  int entry(const pdse_##stem##_desc* d, pdse_stream_t s) { return validate_desc(d) ? 1 : pdse_##stem##_launch(d, (hipStream_t)s); }
PDSE_OPS(X)
#undef X

// the wav back end (csrc/wavout.hip): plain arguments, outside the operator table
int pdse_wav_encode(const float* x, const int32_t* n_in_host, const int32_t* n_keep_host, const int32_t* n_in, const int32_t* n_keep,
                    const double* taps, uint8_t* out, int32_t* clipped, int64_t stride, int32_t B, int32_t Lmax, int32_t up, int32_t down,
                    int32_t half, int32_t fmt, int32_t width, int32_t ch, pdse_stream_t s) {
  return pdse_wavout_launch(x, n_in_host, n_keep_host, n_in, n_keep, taps, out, clipped, stride, B, Lmax, up, down, half, fmt, width, ch,
                            (hipStream_t)s);
}

// the channel encoder of the wav back end (csrc/wavout.hip): ch different rows per file
int pdse_wav_encode_channels(const float* x, const int32_t* n_in_host, const int32_t* n_keep_host, const int32_t* n_in,
                             const int32_t* n_keep, const double* taps, uint8_t* out, int32_t* clipped, int64_t stride, int32_t B,
                             int32_t Lmax, int32_t up, int32_t down, int32_t half, int32_t fmt, int32_t width, int32_t ch, pdse_stream_t s) {
  return pdse_wavch_launch(x, n_in_host, n_keep_host, n_in, n_keep, taps, out, clipped, stride, B, Lmax, up, down, half, fmt, width, ch,
                           (hipStream_t)s);
}

// the validation epoch's pair front end and masked losses (csrc/valid.hip): plain arguments, outside the operator table
int pdse_pair_prep(const float* noisy, const float* clean, const int32_t* lens, float* noisy_pad, float* clean_pad, float* c, int32_t B,
                   int32_t L, int32_t pad, int32_t reflect_own, pdse_stream_t s) {
  return pdse_pair_prep_launch(noisy, clean, lens, noisy_pad, clean_pad, c, B, L, pad, reflect_own, (hipStream_t)s);
}

int pdse_spec_losses(const float* esti, const float* label, const int32_t* frames_host, const int32_t* frames, double* partial,
                     double* per_utt, float* loss, int32_t B, int32_t T, int32_t F, pdse_stream_t s) {
  return pdse_spec_losses_launch(esti, label, frames_host, frames, partial, per_utt, loss, B, T, F, (hipStream_t)s);
}

int pdse_spec_frames(const float* spec, const double* basis, float* frames, int32_t B, int32_t T, int32_t F, pdse_stream_t s) {
  return pdse_spec_frames_launch(spec, basis, frames, B, T, F, (hipStream_t)s);
}
int pdse_spec_frames_mode(const float* spec, const double* basis, float* frames, int32_t B, int32_t T, int32_t F, int32_t mode,
                          pdse_stream_t s) {
  return pdse_spec_frames_mode_launch(spec, basis, frames, B, T, F, mode, (hipStream_t)s);
}

// the denoising objective's forward noising and --sigma loss (csrc/objective.hip): plain arguments, outside the operator table
int pdse_objective_noise(const float* label, const float* init, const float* noise, const int32_t* t, const float* a_tab,
                         const float* s_tab, float* noisy, float* target, float* maxbuf, int32_t B, int32_t T, int32_t F, int32_t mode,
                         int32_t sigma, pdse_stream_t s) {
  return pdse_objective_noise_launch(label, init, noise, t, a_tab, s_tab, noisy, target, maxbuf, B, T, F, mode, sigma, (hipStream_t)s);
}

int pdse_sigma_loss(const float* predicted, const float* target, const float* init, const float* maxbuf, const int32_t* frames_host,
                    const int32_t* frames, double* partial, double* per_utt, float* loss, int32_t B, int32_t T, int32_t F,
                    pdse_stream_t s) {
  return pdse_sigma_loss_launch(predicted, target, init, maxbuf, frames_host, frames, partial, per_utt, loss, B, T, F, (hipStream_t)s);
}

// the statistics of a posterior ensemble (csrc/ensemble.hip): plain arguments, outside the operator table
int pdse_ensemble_stats(const float* members, float* mean, float* spread, const int32_t* frames_host, const int32_t* frames,
                        double* partial, double* per_utt, double* per_member, int32_t K, int32_t B, int32_t T, int32_t F,
                        pdse_stream_t s) {
  return pdse_ensemble_stats_launch(members, mean, spread, frames_host, frames, partial, per_utt, per_member, K, B, T, F, (hipStream_t)s);
}

// gather / scatter of the windowed passes (csrc/window.hip): plain arguments, outside the operator table
int pdse_window_gather(const float* whole, float* win, int32_t B, int32_t C, int32_t T, int32_t F, int32_t W, int32_t a,
                       pdse_stream_t s) {
  return pdse_window_gather_launch(whole, win, B, C, T, F, W, a, (hipStream_t)s);
}

int pdse_window_scatter(const float* win, float* whole, int32_t B, int32_t C, int32_t T, int32_t F, int32_t W, int32_t a,
                        int32_t keep_lo, int32_t keep_hi, pdse_stream_t s) {
  return pdse_window_scatter_launch(win, whole, B, C, T, F, W, a, keep_lo, keep_hi, (hipStream_t)s);
}

int pdse_plan_create(pdse_plan** out) {
  if (!out) {
    pdse_set_error("plan_create: null out");
    return 1;
  }
  *out = new (std::nothrow) pdse_plan();
  if (!*out) {
    pdse_set_error("plan_create: out of memory");
    return 1;
  }
  return 0;
}

int pdse_plan_add(pdse_plan* p, int op_kind, const void* desc, int tag) {
  const int sz = op_size(op_kind);
  if (!p || !desc || sz < 0) {
    pdse_set_error("plan_add: bad argument");
    return 1;
  }
  if (p->exec) {
    pdse_set_error("plan_add: plan already captured into a graph");
    return 1;
  }
  if (op_kind == PDSE_OP_RANGE) {   // the row table is device data: checked once, here, so that a run is launches only
    device_guard dg(p);
    if (!dg.ok || pdse_range_validate(static_cast<const pdse_range_desc*>(desc))) return 1;
  }
  pdse_op op;
  op.kind = op_kind;
  op.tag = tag;
  memcpy(&op.d, desc, (size_t)sz);
  if (check_follows(p, op)) return 1;
  p->ops.push_back(op);
  return 0;
}

int pdse_plan_size(const pdse_plan* p) { return p ? (int)p->ops.size() : -1; }

int pdse_plan_set_device(pdse_plan* p, int device) {
  int n = 0;
  if (!p || device < -1 || (device >= 0 && (hipGetDeviceCount(&n) != hipSuccess || device >= n))) {
    pdse_set_error("plan_set_device: no such device");
    return 1;
  }
  if (p->exec) {
    pdse_set_error("plan_set_device: plan already captured into a graph");
    return 1;
  }
  p->device = device;
  return 0;
}

int pdse_plan_clear(pdse_plan* p) {
  if (!p) {
    pdse_set_error("plan_clear: null plan");
    return 1;
  }
  if (p->exec) (void)hipGraphExecDestroy(p->exec);
  if (p->graph) (void)hipGraphDestroy(p->graph);
  p->exec = nullptr;
  p->graph = nullptr;
  p->ops.clear();
  return 0;
}

int pdse_plan_run_range(pdse_plan* p, int begin, int end, pdse_stream_t s) {
  if (!p || begin < 0 || end > (int)p->ops.size() || begin > end) {
    pdse_set_error("plan_run_range: bad range");
    return 1;
  }
  device_guard dg(p);
  if (!dg.ok) return 1;
  for (int i = begin, n = 1; i < end; i += n)
    if (int rc = launch_at(p, i, end, (hipStream_t)s, &n)) return rc;
  return 0;
}

int pdse_plan_run(pdse_plan* p, pdse_stream_t s) { return pdse_plan_run_range(p, 0, p ? (int)p->ops.size() : 0, s); }

int pdse_plan_build_graph(pdse_plan* p, pdse_stream_t s) {
  if (!p || !s) {
    pdse_set_error("plan_build_graph: needs a plan and a non-default stream");
    return 1;
  }
  if (p->exec) return 0;
  device_guard dg(p);
  if (!dg.ok) return 1;
  hipStream_t st = (hipStream_t)s;
  if (pdse_check_hip(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal), "begin capture")) return 1;
  int rc = pdse_plan_run(p, s);
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(st, &g);
  if (rc) {
    if (g) (void)hipGraphDestroy(g);
    return rc;
  }
  if (pdse_check_hip(e, "end capture")) return 1;
  hipGraphExec_t ex = nullptr;
  if (pdse_check_hip(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0), "graph instantiate")) {
    (void)hipGraphDestroy(g);
    return 1;
  }
  p->graph = g;
  p->exec = ex;
  return 0;
}

int pdse_plan_launch_graph(pdse_plan* p, pdse_stream_t s) {
  if (!p || !p->exec) {
    pdse_set_error("plan_launch_graph: no captured graph");
    return 1;
  }
  device_guard dg(p);
  if (!dg.ok) return 1;
  return pdse_check_hip(hipGraphLaunch(p->exec, (hipStream_t)s), "graph launch");
}

int pdse_plan_time_ops(pdse_plan* p, int begin, int end, pdse_stream_t s, float* ms_out) {
  if (!p || !ms_out || begin < 0 || end > (int)p->ops.size() || begin > end) {
    pdse_set_error("plan_time_ops: bad argument");
    return 1;
  }
  device_guard dg(p);
  if (!dg.ok) return 1;
  hipStream_t st = (hipStream_t)s;
  const int n = end - begin;
  std::vector<hipEvent_t> ev((size_t)n + 1);
  for (auto& e : ev)
    if (pdse_check_hip(hipEventCreate(&e), "event create")) return 1;
  int rc = 0;
  (void)hipEventRecord(ev[0], st);
  for (int i = 0, k = 1; i < n && !rc; i += k) {   // a phase pair is one launch: its time goes to the first operator, 0 to the second
    rc = launch_at(p, begin + i, end, st, &k);
    for (int q = 1; q <= k; ++q) (void)hipEventRecord(ev[i + q], st);
  }
  if (!rc) rc = pdse_check_hip(hipEventSynchronize(ev[n]), "event sync");
  for (int i = 0; i < n && !rc; ++i) rc = pdse_check_hip(hipEventElapsedTime(&ms_out[i], ev[i], ev[i + 1]), "elapsed");
  for (auto& e : ev) (void)hipEventDestroy(e);
  return rc;
}

int pdse_plan_time_tag(pdse_plan* p, int tag, pdse_stream_t s, float* ms_out, int* count_out) {
  if (!p || !ms_out || !count_out) {
    pdse_set_error("plan_time_tag: bad argument");
    return 1;
  }
  device_guard dg(p);
  if (!dg.ok) return 1;
  hipStream_t st = (hipStream_t)s;
  std::vector<hipEvent_t> ev;
  int rc = 0, cnt = 0;
  const int nops = (int)p->ops.size();
  for (int i = 0, k = 1; i < nops && !rc; i += k) {   // count_out counts launches: a phase pair is one
    const bool hit = p->ops[i].tag == tag;
    if (hit) {
      hipEvent_t a, b;
      if (pdse_check_hip(hipEventCreate(&a), "event create") || pdse_check_hip(hipEventCreate(&b), "event create")) {
        rc = 1;
        break;
      }
      (void)hipEventRecord(a, st);
      rc = launch_at(p, i, nops, st, &k);
      (void)hipEventRecord(b, st);
      ev.push_back(a);
      ev.push_back(b);
      ++cnt;
    } else {
      rc = launch_at(p, i, nops, st, &k);
    }
  }
  if (!rc) rc = pdse_check_hip(hipStreamSynchronize(st), "stream sync");
  float total = 0.f;
  for (size_t i = 0; i + 1 < ev.size() && !rc; i += 2) {
    float ms = 0.f;
    rc = pdse_check_hip(hipEventElapsedTime(&ms, ev[i], ev[i + 1]), "elapsed");
    total += ms;
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  *ms_out = total;
  *count_out = cnt;
  return rc;
}

void pdse_plan_destroy(pdse_plan* p) {
  if (!p) return;
  if (p->exec) (void)hipGraphExecDestroy(p->exec);
  if (p->graph) (void)hipGraphDestroy(p->graph);
  for (auto& r : p->regions)
    if (r.ptr) (void)hipFree(r.ptr);
  delete p;
}

// ---- plan files: a recorded plan with everything it points at, for hosts without the Python builders ---------------------------
// Layout (little endian, every item padded to 8 bytes; written by prior-diffuse_amd/planfile.py):
//   "PDSEPLN1" | u32 abi | u32 nregions | u32 nops | u32 0
//   region: u64 old_base | u64 bytes | u32 kind (low byte: 0 scratch, 1 zeroed, 2 data follows; bits 8..: element type, for
//           readers that want typed views - ignored here) | u32 name_len | name | [data]
//   op:     i32 kind | i32 tag | u32 desc_size | u32 nptr | u32 offsets[nptr] | descriptor bytes
// Loading allocates every region on the current device (or the plan's), uploads / zeroes it and rebases the pointer fields of
// every descriptor (listed by offset) from the recorded addresses to the new ones.
}   // extern "C"
namespace {
struct reader {
  FILE* f;
  bool ok = true;
  void get(void* dst, size_t n) {
    if (ok && fread(dst, 1, n, f) != n) ok = false;
  }
  void skip_pad(size_t n) {
    const size_t pad = (8 - (n & 7)) & 7;
    char z[8];
    if (pad) get(z, pad);
  }
  template <typename T>
  T val() {
    T v{};
    get(&v, sizeof(T));
    return v;
  }
};
}  // namespace
extern "C" {

int pdse_plan_load(const char* path, pdse_plan** out) {
  if (!path || !out) {
    pdse_set_error("plan_load: null argument");
    return 1;
  }
  FILE* f = fopen(path, "rb");
  if (!f) {
    pdse_set_error("plan_load: cannot open the file");
    return 1;
  }
  reader rd{f};
  pdse_plan* p = new (std::nothrow) pdse_plan();
  auto fail = [&](const char* msg) {
    pdse_set_error(msg);
    fclose(f);
    pdse_plan_destroy(p);
    return 1;
  };
  if (!p) return fail("plan_load: out of memory");
  char magic[8];
  rd.get(magic, 8);
  const uint32_t abi = rd.val<uint32_t>(), nreg = rd.val<uint32_t>(), nops = rd.val<uint32_t>();
  (void)rd.val<uint32_t>();
  if (!rd.ok || memcmp(magic, "PDSEPLN1", 8) != 0) return fail("plan_load: not a plan file");
  if (abi != PDSE_ABI_VERSION) return fail("plan_load: the file was written for another ABI version");
  if (nreg > (1u << 20) || nops > (1u << 22)) return fail("plan_load: implausible header");
  std::vector<uint64_t> old_base(nreg);
  std::vector<char> buf;
  for (uint32_t i = 0; i < nreg; ++i) {
    pdse_region r;
    old_base[i] = rd.val<uint64_t>();
    r.bytes = rd.val<uint64_t>();
    const uint32_t kind = rd.val<uint32_t>() & 0xffu, nlen = rd.val<uint32_t>();
    if (!rd.ok || nlen > 256 || kind > 2 || r.bytes == 0 || r.bytes > (1ull << 40)) return fail("plan_load: bad region record");
    r.name.resize(nlen);
    rd.get(&r.name[0], nlen);
    rd.skip_pad(nlen);
    if (pdse_check_hip(hipMalloc(&r.ptr, r.bytes), "plan_load: hipMalloc")) return fail(pdse_last_error());
    p->regions.push_back(r);   // owned from here on (freed by destroy)
    if (kind == 2) {
      buf.resize(r.bytes);
      rd.get(buf.data(), r.bytes);
      rd.skip_pad(r.bytes);
      if (!rd.ok) return fail("plan_load: truncated region data");
      if (pdse_check_hip(hipMemcpy(r.ptr, buf.data(), r.bytes, hipMemcpyHostToDevice), "plan_load: upload")) return fail(pdse_last_error());
    } else {
      if (pdse_check_hip(hipMemset(r.ptr, 0, r.bytes), "plan_load: memset")) return fail(pdse_last_error());
    }
  }
  // a recorded address becomes the same offset into the region that held it; false when no region did
  auto rebase = [&](uint64_t& v) {
    for (uint32_t r = 0; r < nreg; ++r) {
      if (v >= old_base[r] && v < old_base[r] + p->regions[r].bytes) {
        v = reinterpret_cast<uint64_t>(p->regions[r].ptr) + (v - old_base[r]);
        return true;
      }
    }
    return false;
  };
  std::vector<uint32_t> offs;
  for (uint32_t i = 0; i < nops; ++i) {
    pdse_op op;
    op.kind = rd.val<int32_t>();
    op.tag = rd.val<int32_t>();
    const uint32_t dsz = rd.val<uint32_t>(), nptr = rd.val<uint32_t>();
    const int want = op_size(op.kind);
    if (!rd.ok || want < 0 || (uint32_t)want != dsz || nptr > dsz / 8) return fail("plan_load: bad operator record (descriptor size or kind)");
    offs.resize(nptr);
    rd.get(offs.data(), nptr * sizeof(uint32_t));
    rd.skip_pad(nptr * sizeof(uint32_t));
    memset(&op.d, 0, sizeof(op.d));
    rd.get(&op.d, dsz);
    rd.skip_pad(dsz);
    if (!rd.ok) return fail("plan_load: truncated operator record");
    char* const base = reinterpret_cast<char*>(&op.d);
    for (uint32_t k = 0; k < nptr; ++k) {
      if (offs[k] + 8 > dsz || (offs[k] & 7)) return fail("plan_load: bad pointer offset");
      uint64_t v;
      memcpy(&v, base + offs[k], 8);
      if (!v) continue;
      if (!rebase(v)) return fail("plan_load: a descriptor points outside every recorded region");
      memcpy(base + offs[k], &v, 8);
    }
    if (check_follows(p, op)) {
      const std::string why = pdse_last_error();
      return fail(why.c_str());
    }
    p->ops.push_back(op);
  }
  // The row table of a range audit (PDSE_OP_RANGE) is device data that holds device pointers: rebase them like descriptor
  // fields.  Every accumulate op of a plan may share one table, so a table is rewritten once; the rebased table is then
  // validated like a recorded one.
  std::vector<const void*> tables_done;
  for (auto& op : p->ops) {
    if (op.kind != PDSE_OP_RANGE) continue;
    pdse_range_desc& rd_ = op.d.range;
    if (!rd_.rows || rd_.nrows < 1 || rd_.nrows > 65535) continue;
    bool done = false;
    for (const void* t : tables_done) done = done || t == rd_.rows;
    if (done) continue;
    std::vector<pdse_range_row> rows((size_t)rd_.nrows);
    if (pdse_check_hip(hipMemcpy(rows.data(), rd_.rows, rows.size() * sizeof(pdse_range_row), hipMemcpyDeviceToHost), "plan_load: range table")) return fail(pdse_last_error());
    for (auto& row : rows) {
      uint64_t v = reinterpret_cast<uint64_t>(row.ptr);
      if (!rebase(v)) return fail("plan_load: a range-audit row points outside every recorded region");
      row.ptr = reinterpret_cast<const void*>(v);
    }
    if (pdse_check_hip(hipMemcpy(const_cast<pdse_range_row*>(rd_.rows), rows.data(), rows.size() * sizeof(pdse_range_row), hipMemcpyHostToDevice), "plan_load: range table")) return fail(pdse_last_error());
    tables_done.push_back(rd_.rows);
    if (pdse_range_validate(&rd_)) return fail(pdse_last_error());
  }
  fclose(f);
  *out = p;
  return 0;
}

int pdse_plan_region(const pdse_plan* p, const char* name, void** ptr, uint64_t* nbytes) {
  if (!p || !name || !ptr) {
    pdse_set_error("plan_region: null argument");
    return 1;
  }
  for (const auto& r : p->regions) {
    if (r.name == name) {
      *ptr = r.ptr;
      if (nbytes) *nbytes = r.bytes;
      return 0;
    }
  }
  pdse_set_error("plan_region: no region of that name in this plan (plans recorded in this process keep their buffers in the caller)");
  return 1;
}

// copy inputs into the plan's named regions, run it, copy the named outputs out - all on stream s, device to device
static int plan_call(pdse_plan* p, const int n_in, const char* const* in_names, const void* const* in_ptrs, const int n_out,
                     const char* const* out_names, void* const* out_ptrs, pdse_stream_t s) {
  if (!p) {
    pdse_set_error("forward: null plan");
    return 1;
  }
  device_guard dg(p);
  if (!dg.ok) return 1;
  for (int i = 0; i < n_in; ++i) {
    if (!in_ptrs[i]) continue;   // optional input left as the plan holds it
    void* dst;
    uint64_t n;
    if (pdse_plan_region(p, in_names[i], &dst, &n)) return 1;
    if (pdse_check_hip(hipMemcpyAsync(dst, in_ptrs[i], n, hipMemcpyDeviceToDevice, (hipStream_t)s), "forward: input copy")) return 1;
  }
  if (pdse_plan_run(p, s)) return 1;
  for (int i = 0; i < n_out; ++i) {
    if (!out_ptrs[i]) continue;
    void* src;
    uint64_t n;
    if (pdse_plan_region(p, out_names[i], &src, &n)) return 1;
    if (pdse_check_hip(hipMemcpyAsync(out_ptrs[i], src, n, hipMemcpyDeviceToDevice, (hipStream_t)s), "forward: output copy")) return 1;
  }
  return 0;
}

int pdse_prior_forward(pdse_plan* p, const float* feat, float* x_init, pdse_stream_t s) {
  const char* in[] = {"x"};
  const void* ip[] = {feat};
  const char* on[] = {"out"};
  void* op[] = {x_init};
  return plan_call(p, 1, in, ip, 1, on, op, s);
}

int pdse_eps_forward(pdse_plan* p, const float* x, const float* x_init, const float* t, float* eps, pdse_stream_t s) {
  const char* in[] = {"x", "x_init", "t"};
  const void* ip[] = {x, x_init, t};
  const char* on[] = {"out"};
  void* op[] = {eps};
  return plan_call(p, 3, in, ip, 1, on, op, s);
}

int pdse_enhance(pdse_plan* p, const float* wav, const float* x_T, float* wav_out, float* spec_out, pdse_stream_t s) {
  const char* in[] = {"wav", "x_T"};
  const void* ip[] = {wav, x_T};
  const char* on[] = {"wav_out", "spec"};
  void* op[] = {wav_out, spec_out};
  return plan_call(p, 2, in, ip, 2, on, op, s);
}

}  // extern "C"
