// anatomix_amd -- host-side declarations shared between translation units: the amx:: functions that one .hip file defines and
// ANOTHER calls, with their default arguments.  A C ABI entry lives in the file that defines the launcher it calls;
// a launcher that only its own file calls is `static` there, carries its default arguments at its definition and is not declared
// here (tests/test_launch_header.py holds this header and amx_gemm.h to that).  Also here: the error helper of the C ABI entries, their
// shared checks, the cached CU count of a device and the one statement of the stored tensor layouts (the stride setters at the end).
// The conv launchers keep no state between calls: what a launch ran, and how many statistics slots it wrote, comes back through the
// caller's ConvLaunchInfo.
// Not part of the public C ABI (that is include/anatomix_amd.h).  The ViT engine's launchers and parameter structs are in amx_gemm.h.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include <functional>

#include "../../include/anatomix_amd.h"
#include "amx_common.h"

namespace amx {

// What a conv launcher ran, for the callers that ask (null: nothing is formatted).  name: as in amx_launch_record::kernel; stats_slots:
// partial-statistics slots per sample that the launch writes into ConvParams::stats, 0 when that is null.  A launcher reports both at once.
struct ConvLaunchInfo {
  char name[64];
  int stats_slots;
  __attribute__((format(printf, 3, 4))) void report(int slots, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name, sizeof name, fmt, ap);
    va_end(ap);
    stats_slots = slots;
  }
};

// amx_conv3d.hip
hipError_t launch_conv(const ConvParams& p, int precision, int Q, hipStream_t st, ConvLaunchInfo* info = nullptr);
hipError_t launch_pack_weights(const float* w, const float* scale, void* wpk, int CinReal, int CinPad,
                               int Cout, int Q, int precision, hipStream_t st, int mode = 0, int CoutReal = 0, int CinStride = 0,
                               int C0Real = 0, int C0Phys = 0);
hipError_t launch_pack_weights_batch(int count, const float* const* w, void* const* wpk, const int* CinReal, const int* CinPad, const int* Cout,
                                     const int* Q, const int* mode, const int* CoutReal, int precision, hipStream_t st);
hipError_t launch_pack_weights_mx(const float* w, const float* scale, void* wpk, int* mxs, int CinReal, int CinPad, int Cout, int Q,
                                  hipStream_t st, int CoutReal = 0, int CinStride = 0, int C0Real = 0, int C0Phys = 0);
hipError_t launch_fold_norm(const float* gamma, const float* beta, const float* mean, const float* var,
                            const float* conv_bias, float eps, int C, float* scale, float* shift,
                            hipStream_t st);
hipError_t launch_pool2(const void* in, void* out, int N, int Do, int Ho, int Wo, int C, int avg,
                        int precision, hipStream_t st, int skip_lo = 0);
int conv_pick_q(int Cout, int W, int precision);
bool conv_fuses_stats(const ConvParams& p, int precision, int Q);

// amx_conv3d_v2.hip
int conv_v2_stats_slots(int D, int H, int W, int Q);
hipError_t launch_conv_v2(const ConvParams& p, int precision, int Q, hipStream_t st, ConvLaunchInfo* info = nullptr);

// amx_conv3d_ks.hip
size_t conv_ks_part_bytes(int C0, int Cout, int N, int D, int H, int W, int precision, int Q);
bool conv_ks_eligible(const ConvParams& p, int precision, int Q);
hipError_t launch_conv_ks(const ConvParams& p, int precision, int Q, hipStream_t st, ConvLaunchInfo* info = nullptr);

// amx_conv3d_zmarch.hip
bool conv_zmarch_can_pool(const ConvParams& p);
bool conv_zmarch_can_pool_split(const ConvParams& p);
bool conv_zmarch_eligible(const ConvParams& p);
bool conv_zmarch_stem_eligible(const ConvParams& p, int precision);
hipError_t launch_conv_zmarch_stem(const ConvParams& p, const float* x, long long xs_n, long long xs_z, long long xs_y, const long long* x_offs,
                                   const void* stem_wpk, const float* stem_bias, int stem_act, float stem_slope, int precision, hipStream_t st,
                                   ConvLaunchInfo* info = nullptr);
bool conv_zmarch_eligible_split(const ConvParams& p);
hipError_t launch_conv_zmarch(const ConvParams& p, int precision, hipStream_t st, ConvLaunchInfo* info = nullptr);

// amx_conv3d_zx.hip
bool conv_zx_shape_eligible(const ConvParams& p);     // shapes only: p.out is not asked, its strides are
size_t conv_zx_packed_bytes();
hipError_t launch_pack_weights_zx(const float* w, const float* scale, void* wx, const int* mxs, int CoutReal, hipStream_t st);
hipError_t launch_conv_zx(ConvParams p, const float* in_ab, int in_act, float in_slope, const void* wx, hipStream_t st, ConvLaunchInfo* info = nullptr);

// amx_conv3d_stem.hip
hipError_t launch_conv_stem(const ConvParams& p, int precision, hipStream_t st, ConvLaunchInfo* info = nullptr);
hipError_t launch_pack_stem(const float* w, const float* scale, void* wpk, int Cout, int precision, hipStream_t st, int CoutReal = 0);
int conv_stem_stats_slots(const ConvParams& p, int precision);

// amx_conv3d_upcat.hip
size_t conv_upcat16_packed_bytes();
bool conv_upcat16_eligible(const ConvParams& p);
hipError_t launch_conv_upcat16(const ConvParams& p, int precision, hipStream_t st, ConvLaunchInfo* info = nullptr);
hipError_t launch_pack_upcat16(const float* w, const float* scale, void* wpk, int precision, hipStream_t st);

// amx_conv3d_upmerge.hip
size_t conv_upmerge_packed_bytes(int C1, int Cout, int split);
bool conv_upmerge_eligible(int C0, int C1, int Cout, int D, int H, int W, int up_shift, int split);
hipError_t launch_conv_upmerge(const UpmergeParams& p, int precision, hipStream_t st, ConvLaunchInfo* info = nullptr);
hipError_t launch_pack_upmerge(const float* w, const float* scale, void* wpk, int c_off, int CinTotal, int C1, int Cout, int precision,
                               hipStream_t st);

// amx_norm.hip
size_t instnorm_scratch_bytes(int N, int C, long long max_slots_x_C);
bool in_apply_pool_eligible(int precision, int D, int H, int W, int C);
hipError_t launch_in_apply_pool(void* x, const float* ab, void* pooled, int N, int D, int H, int W, int C, int act, float slope, int avg,
                                int skip_lo, int pool_skip_lo, int* oflow, hipStream_t st);
hipError_t launch_instnorm(void* x, const float* gamma, const float* beta, float eps, int N, long long vox, int C, int act,
                           float slope, void* scratch, int precision, hipStream_t st, int* oflow = nullptr, int fused_slots = 0,
                           const float* kshift = nullptr, int W = 0, int skip_lo = 0, int apply = 1, float* ab_out = nullptr);
hipError_t launch_poison_if_flag(const int* flag, int* host_flag, float* y, long long count, hipStream_t st);
hipError_t launch_upsample2_trilinear(const void* in, void* out, int N, int D, int H, int W, int C, int precision,
                                      hipStream_t st, int skip_lo = 0, const float* ab = nullptr, int act = 0, float slope = 0.f,
                                      int* oflow = nullptr);
hipError_t launch_affine_act(void* x, const float* scale, const float* shift, int N, long long vox, int C, int act,
                             float slope, int precision, hipStream_t st, int* oflow = nullptr);
hipError_t launch_export_ncdhw(const void* src0, int C0, const void* src1, int C1, int up_shift, int N, int D, int H, int W,
                               float* out, int precision, hipStream_t st, int S0 = 0, int S1 = 0);
hipError_t launch_import_input(const float* src, void* dst, int N, int Cin, long long vox, int precision, hipStream_t st);

// amx_sw.hip
// The window schedule of one axis (registration/sliding_window.py window_starts): start i = min(i * interval, size - roi) for
// i in [0, count).  The one statement of that arithmetic: amx_sw_plan lists the corners from it, the count-map kernel walks it.
struct SwAxis {
  int size, roi, interval, count;
  __host__ __device__ int start(int i) const { return i * interval < size - roi ? i * interval : size - roi; }
};
struct SwPlan {
  SwAxis ax[3];      // z, y, x
  int windows() const { return ax[0].count * ax[1].count * ax[2].count; }
  void corner(int i, int* zyx) const {      // window i in MONAI's order: first axis outermost
    zyx[2] = ax[2].start(i % ax[2].count);
    zyx[1] = ax[1].start(i / ax[2].count % ax[1].count);
    zyx[0] = ax[0].start(i / (ax[2].count * ax[1].count));
  }
};
constexpr int kSwMaxWindows = 1 << 20;         // a plan holds no more windows than this
constexpr int kSwMaxF = 64, kSwMaxC = 32;      // the head envelope of sw_finish: amx_seg_argmax's (amx_segloss.hip)
// off[i] = where window i of offsets_zyx[n][3] starts in a [vd][vh][vw] volume, in voxels; AMX_ERR_SHAPE when a window leaves the volume
int sw_window_offsets(int vd, int vh, int vw, int rd, int rh, int rw, int n, const int* offsets_zyx, long long* off);
// The window weights of the last (roi, mode, sigma_scale) on a network handle, created at first use.  fetch: `map` holds this key's
// weights once `st` gets there -- built on `st` when the key is new, else the build is waited for.
struct SwMapCache {
  float* map = nullptr;
  int roi[3] = {0, 0, 0}, mode = -1;
  double sigma = 0.0;
  hipEvent_t ready = nullptr;
  int fetch(int rd, int rh, int rw, int mode, double sigma_scale, hipStream_t st);
  void release();
};
// The second lane of a call that keeps two window batches in flight (lane 0 is the caller's stream) and the events that fork it from and
// join it to the caller's, created at first use
struct SwLanes {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  void release();
};
// A network as sw_run sees it.  check: everything the network refuses for batches of k windows, launching nothing.  run: enqueues the
// windows offs[nw][3] on `st`; slot 0 / 1 = the lane of a two-lane call (accumulations gated on the other slot's), -1 = one lane.
constexpr int kSwMaxBatch = 64;
struct SwNet {
  const char *entry, *prefix;      // the C entry's name and what the network's messages start with
  int channels, max_batch, roi[3];
  int lane_groups;                 // two lanes from this many window batches on (0: one stream always)
  std::function<int(int k)> check;
  std::function<int(int nw, const int* offs, int slot, hipStream_t st)> run;
};
// plan -> window weights -> count map -> window batches -> finish on `st`, every other batch on lanes->stream when the network asks for
// two lanes (lanes may be null otherwise).  Every refusal comes before the first launch.
int sw_run(const SwNet& net, SwMapCache& cache, SwLanes* lanes, int vd, int vh, int vw, double overlap, int mode, double sigma_scale, int n_batch,
           int out_kind, const float* d_w, const float* d_b, int classes, float* d_acc, float* d_cnt, void* d_out, hipStream_t st);

// amx_mlp.hip
hipError_t launch_small_gemm_batch(int nb, bool ta, bool tb, const float* const* A, const float* const* B, float* const* Cm, int M,
                                   int N, int R, int splits, float scale, hipStream_t st);

// amx_regfeat.hip
hipError_t launch_pool_cat(const float* a, int ca, float sa, const float* b, int cb, float sb, int H, int W, int D, int g,
                           float* out, hipStream_t st);
hipError_t launch_box_filter(const float* in, float* out, int C, int H, int W, int D, int k, hipStream_t st);
size_t correlate_scratch_bytes(int h, int w, int d, int disp_hw);
hipError_t launch_correlate(const float* fix, const float* mov, int C, int h, int w, int d, int disp_hw, float* ssd,
                            long long* argmin, void* scratch, hipStream_t st);

// amx_regsolve.hip
hipError_t launch_resize_trilinear(const float* in, int C, int h, int w, int d, float* out, int H, int W, int D,
                                   const float* scale, int flip, hipStream_t st);

// amx_segaug.hip: the min / max of n rows of V floats (CLIP: of max(x, 0)) as per-workgroup partial pairs in `scratch`
// (minmax_bytes)
size_t minmax_bytes(int n, long long V);
hipError_t launch_minmax_partials(const float* x, int n, long long V, bool clip, void* scratch, hipStream_t st);

// amx_attention.hip
size_t attention_scratch_bytes(int b, int heads, int n);
void attention_operands(void* scratch, int b, int heads, int n, void** Qp, void** Kp, void** Vt, int* npad_out, int* nblk_pad_out);
hipError_t launch_attention_fwd(const void* Qp, const void* Kp, const void* Vt, int b, int n, int heads, int hd, float* out, hipStream_t st,
                                float* lse = nullptr);     // lse: [b][heads][n] log-sum-exp (exp2 domain) for the backward, or null

// amx_api.hip: stores the thread-local message that amx_last_error() returns, and gives `code` back
int fail(int code, const char* fmt, ...);
// the scratch check of the C ABI entries: AMX_OK, or AMX_ERR_WORKSPACE when the caller's `got` bytes are fewer than `need`
inline int need_scratch(size_t need, size_t got) {
  return got < need ? fail(AMX_ERR_WORKSPACE, "scratch needs %zu bytes (got %zu)", need, got) : AMX_OK;
}

// the checks of the row-streaming C ABI units (amx_segaug.hip, amx_preaug.hip, amx_synth.hip).  A unit names its rows: `count` is
// the argument ("n", "views", "rows"), `one` a single row ("sample", "view", "row").
constexpr long long kMaxRowVoxels = 1LL << 31;      // per row: keeps every tile count inside an int
inline bool row_count_ok(int n) { return n >= 1 && n <= 65535; }      // rows are grid.y
inline bool row_voxels_ok(long long voxels) { return voxels >= 1 && voxels < kMaxRowVoxels; }
inline bool rows_ok(int n, long long voxels) { return row_count_ok(n) && row_voxels_ok(voxels); }
inline int check_rows(int n, long long voxels, const char* count, const char* one) {
  if (!row_count_ok(n)) return fail(AMX_ERR_SHAPE, "1 <= %s <= 65535 (got %d)", count, n);
  if (!row_voxels_ok(voxels)) return fail(AMX_ERR_SHAPE, "1 <= voxels < 2^31 per %s (got %lld)", one, voxels);
  return AMX_OK;
}
inline int check_rows_dims(int n, int d, int h, int w, const char* count, const char* one) {
  if (d < 1 || h < 1 || w < 1) return fail(AMX_ERR_SHAPE, "spatial sizes must be positive (got %d x %d x %d)", d, h, w);
  return check_rows(n, (long long)d * h * w, count, one);
}
inline int check_tables(const void* h_table, const void* d_table) {
  if (!h_table || !d_table) return fail(AMX_ERR_INVALID, "null parameter table (host copy and device copy are both needed)");
  return AMX_OK;
}
inline bool is_finite(float v) { return v == v && v - v == 0.f; }
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// precision helpers of the C ABI units (amx_api.hip, amx_unet.hip; kept here so that the two share one copy)
// strict precision (AMX_PREC_F16X2 / AMX_PREC_BF16X2): every stored voxel holds [hi(C) | lo(C)] 16-bit channels
// AMX_PREC_F16X2_MX: the pair plus 2 bytes of e4m3 copies per channel (amx_common.h, voxel layout FMT 2)
inline bool is_split(int precision) { return precision >= AMX_PREC_F16X2; }
inline bool is_mx(int precision) { return precision == AMX_PREC_F16X2_MX; }
inline long long elem_bytes(int precision) { return fmt_elem_bytes(fmt_of_precision(precision)); }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// compute units of device `dev` -- the current one, as the launcher's DeviceOnce has just read it -- asked once per device ordinal
// (0: the runtime could not say); sizes the persistent grids
inline int device_cus(int dev) {
  static int cus[64] = {};
  hipDeviceProp_t prop;
  if (dev >= 0 && dev < 64 && cus[dev]) return cus[dev];
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
  const int n = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (dev >= 0 && dev < 64) cus[dev] = n;
  return n;
}

// ---- the stored tensor layouts (amx_common.h, FMT 0 / 1 / 2), stated once: the byte strides of a dense [N][D][H][W][C] tensor; returns
// the bytes between a voxel's 16-channel chunks.  A row is C * elem_bytes * W bytes in every layout.  Channels-last voxels (all but
// f16x2mx): x = one voxel, chunks 32 bytes apart.  Row-planar (f16x2mx): 32 bytes per voxel inside a row plane, chunks W * 32 apart.
inline int dense_strides(int C, int D, int H, int W, int precision, long long& n, long long& z, long long& y, long long& x) {
  const long long voxel = (long long)C * elem_bytes(precision);
  x = is_mx(precision) ? 32 : voxel; y = voxel * W; z = y * H; n = z * D;
  return is_mx(precision) ? W * 32 : 32;
}
// the input segments of a conv or weight-gradient launch, each at its OWN extents (a half-resolution src1: D / 2, H / 2, W / 2)
template <typename P>
inline void set_src0(P& p, const void* ptr, int C, int D, int H, int W, int precision) {
  p.src0 = (const char*)ptr; p.C0 = C;
  const int cs = dense_strides(C, D, H, W, precision, p.s0n, p.s0z, p.s0y, p.s0x);
  if constexpr (__is_same(P, ConvParams)) p.cs0 = cs;        // (WgradParams: channels-last only)
}
template <typename P>
inline void set_src1(P& p, const void* ptr, int C, int D, int H, int W, int precision) {
  p.src1 = (const char*)ptr; p.C1 = C;
  const int cs = dense_strides(C, D, H, W, precision, p.s1n, p.s1z, p.s1y, p.s1x);
  if constexpr (__is_same(P, ConvParams)) p.cs1 = cs;
}
// the 16-bit output of a conv launch; the max-pooled second output of the z-march kernels at ITS extents (channels-last: those kernels
// have no row-planar form); the low-resolution source of a merged-tap launch
inline void set_out(ConvParams& p, void* ptr, int C, int D, int H, int W, int precision) {
  p.out = (char*)ptr;
  p.ocs = dense_strides(C, D, H, W, precision, p.on, p.oz, p.oy, p.ox);
}
inline void set_out2(ConvParams& p, void* ptr, int C, int D, int H, int W, int precision) {
  p.out2 = (char*)ptr;
  dense_strides(C, D, H, W, precision, p.qn, p.qz, p.qy, p.qx);
}
inline void set_src(UpmergeParams& u, const void* ptr, int C, int D, int H, int W, int precision) {
  u.src = (const char*)ptr; u.C1 = C;
  u.cs = dense_strides(C, D, H, W, precision, u.sn, u.sz, u.sy, u.sx);
}

}  // namespace amx

#define AMX_HIP(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return amx::fail(AMX_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
