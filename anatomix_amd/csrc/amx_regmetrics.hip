// anatomix_amd -- the two figures a registration run reports (anatomix/registration):
//   label overlap counts, from which the driver's macro Dice follows      run_convex_adam_with_network_feats.py:283-295
//   the Jacobian determinant of the fitted map and its statistics         convex_adam_utils.py:226-282 (generate_grid, JacobianDet)
// fp32 or integer data, planar, batch 1, on the caller's stream without host synchronisation or allocation.  Both are single-pass
// streaming kernels.  The counts are integers added with integer atomics (adds commute: exact and reproducible); the Jacobian's
// sums cross workgroups through a partial slab in the caller's scratch that a last one-workgroup launch merges in a fixed order in
// double, as in amx_segloss.hip: no float atomics, results are bit-identical from run to run.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "amx_device.h"
#include "amx_launch.h"
#include "amx_stream.h"

// no fused multiply-add contraction: the determinant has the same bits whichever instantiation computes it (with or without the
// statistics), and each product is rounded as the reference's fp32 arithmetic rounds it
#pragma clang fp contract(off)

namespace amx {

constexpr int kRmThreads = 256, kRmWaves = kRmThreads / 64;
constexpr int kLovMaxBins = 1024;
constexpr int kLovUnroll = 4;              // quads a thread loads before it counts any: the loads of a turn are all in flight together

enum { RM_LABEL_F32 = 0, RM_LABEL_I64 = 1, RM_LABEL_U8 = 2 };       // = AMX_SEG_LABEL_*

// ---- label overlap ----------------------------------------------------------------------------------------------------------
// bin of one label, -1 when it is not an integer in [0, bins): a fractional, negative, NaN or too large value.  A float label is
// compared, never truncated; the bin is only formed after the range check.
__device__ __forceinline__ int lov_bin(float f, int bins) { return (f >= 0.f && f < (float)bins && f == (float)(int)f) ? (int)f : -1; }
__device__ __forceinline__ int lov_bin(long long l, int bins) { return (l >= 0 && l < bins) ? (int)l : -1; }
__device__ __forceinline__ int lov_bin(unsigned u, int bins) { return u < (unsigned)bins ? (int)u : -1; }

template <int LT>
__device__ __forceinline__ int lov_load1(const void* __restrict__ p, long long i, int bins) {
  if (LT == RM_LABEL_F32) return lov_bin(((const float*)p)[i], bins);
  if (LT == RM_LABEL_I64) return lov_bin(((const long long*)p)[i], bins);
  return lov_bin((unsigned)((const unsigned char*)p)[i], bins);
}

// the four labels of quad q behind 16-byte loads (one for fp32, two for int64; a uint8 quad is one 4-byte load).  p is aligned to
// the access size.
template <int LT>
__device__ __forceinline__ void lov_load4(const void* __restrict__ p, long long q, int bins, int (&l)[4]) {
  if (LT == RM_LABEL_F32) {
    const f32x4 v = ((const f32x4*)p)[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) l[j] = lov_bin(v[j], bins);
  } else if (LT == RM_LABEL_I64) {
    typedef __attribute__((ext_vector_type(2))) long long i64x2;
    const i64x2 v0 = ((const i64x2*)p)[2 * q], v1 = ((const i64x2*)p)[2 * q + 1];
    l[0] = lov_bin(v0[0], bins), l[1] = lov_bin(v0[1], bins), l[2] = lov_bin(v1[0], bins), l[3] = lov_bin(v1[1], bins);
  } else {
    const unsigned v = ((const unsigned*)p)[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) l[j] = lov_bin((v >> (8 * j)) & 255u, bins);
  }
}
template <int LT>
constexpr int lov_elem_bytes() { return LT == RM_LABEL_F32 ? 4 : (LT == RM_LABEL_I64 ? 8 : 1); }
template <int LT>
constexpr int lov_quad_align() { return LT == RM_LABEL_U8 ? 4 : 16; }

// key = bin of a | bin of b << 16 (bins <= 1024): n voxels of that pair into the workgroup's histogram [bins][3]
__device__ __forceinline__ void lov_add(unsigned* __restrict__ hist, int key, unsigned n) {
  const int la = key & 0xffff, lb = key >> 16;
  atomicAdd(&hist[3 * la], n);
  atomicAdd(&hist[3 * lb + 1], n);
  if (la == lb) atomicAdd(&hist[3 * la + 2], n);
}

__global__ __launch_bounds__(kRmThreads) void label_overlap_zero_kernel(unsigned long long* __restrict__ counts, int n,
                                                                        unsigned long long* __restrict__ bad) {
  const int i = blockIdx.x * kRmThreads + threadIdx.x;
  if (i < n) counts[i] = 0;
  if (i == 0) *bad = 0;
}

// Voxels [head, head + 4 nq) are read as quads (a + head and b + head are aligned for that), the `voxels - 4 nq` others one by
// one.  The grid is min(what the work needs, kStreamMaxBlocks), so a workgroup sees at most voxels / kStreamMaxBlocks + 8192 voxels: with
// voxels < 2^40 that is below 2^30, and its 32-bit LDS counters cannot wrap before the one flush at the end.
template <int LA, int LB>
__global__ __launch_bounds__(kRmThreads) void label_overlap_kernel(const void* __restrict__ a, const void* __restrict__ b, long long head,
                                                                   long long nq, long long voxels, int bins,
                                                                   unsigned long long* __restrict__ counts,
                                                                   unsigned long long* __restrict__ bad_out) {
  __shared__ unsigned hist[3 * kLovMaxBins];
  __shared__ unsigned long long badred[kRmWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 3 * bins; i += kRmThreads) hist[i] = 0;
  __syncthreads();
  unsigned long long bad = 0;
  const void* av = (const char*)a + head * lov_elem_bytes<LA>();
  const void* bv = (const char*)b + head * lov_elem_bytes<LB>();
  const long long stride = (long long)gridDim.x * kRmThreads;
  for (long long q0 = (long long)blockIdx.x * kRmThreads * kLovUnroll; q0 < nq; q0 += stride * kLovUnroll) {      // uniform across the workgroup
    int k[kLovUnroll][4];
#pragma unroll
    for (int u = 0; u < kLovUnroll; ++u) {
      const long long q = q0 + u * kRmThreads + tid;
      if (q < nq) {
        int la[4], lb[4];
        lov_load4<LA>(av, q, bins, la);
        lov_load4<LB>(bv, q, bins, lb);
#pragma unroll
        for (int j = 0; j < 4; ++j) k[u][j] = (la[j] | lb[j]) < 0 ? -1 : (la[j] | (lb[j] << 16));
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) k[u][j] = -2;
      }
    }
#pragma unroll
    for (int u = 0; u < kLovUnroll; ++u) {
      const bool active = k[u][0] != -2;
      const int first = __builtin_amdgcn_readfirstlane(k[u][0]);  // lane 0: every lane is here, the loop bounds are uniform
      if (first == -2) continue;                                   // the whole wave lies past the end
      const bool mine = k[u][0] == k[u][1] && k[u][1] == k[u][2] && k[u][2] == k[u][3];
      const unsigned n = 4u * (unsigned)__popcll(__ballot(active));
      if (__all(!active || (mine && k[u][0] == first))) {
        // label maps are spatially coherent: the wave's 4 x (active lanes) voxels are one (a, b) pair -> one add of their number
        if (lane == 0) {
          if (first < 0) bad += n;
          else lov_add(hist, first, n);
        }
      } else if (active) {
        if (mine) {
          if (k[u][0] < 0) bad += 4;
          else lov_add(hist, k[u][0], 4u);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (k[u][j] < 0) ++bad;
            else lov_add(hist, k[u][j], 1u);
          }
        }
      }
    }
  }
  const long long rest = voxels - 4 * nq;
  for (long long e = (long long)blockIdx.x * kRmThreads + tid; e < rest; e += stride) {
    const long long i = e < head ? e : e + 4 * nq;
    const int la = lov_load1<LA>(a, i, bins), lb = lov_load1<LB>(b, i, bins);
    if ((la | lb) < 0) ++bad;
    else lov_add(hist, la | (lb << 16), 1u);
  }
  bad = wave_reduce_xor<SumOp>(bad);
  if (lane == 0) badred[wave] = bad;
  __syncthreads();
  if (tid == 0) {
    unsigned long long s = 0;
    for (int w = 0; w < kRmWaves; ++w) s += badred[w];
    if (s) atomicAdd(bad_out, s);
  }
  for (int i = tid; i < 3 * bins; i += kRmThreads) {
    const unsigned v = hist[i];
    if (v) atomicAdd(&counts[i], (unsigned long long)v);
  }
}

template <int LT>
static inline bool lov_aligned(const void* p, long long head) {
  return (((uintptr_t)p + (uintptr_t)head * lov_elem_bytes<LT>()) & (lov_quad_align<LT>() - 1)) == 0;
}
static inline bool lov_aligned_dyn(int lt, const void* p, long long head) {
  return lt == RM_LABEL_F32 ? lov_aligned<RM_LABEL_F32>(p, head) : (lt == RM_LABEL_I64 ? lov_aligned<RM_LABEL_I64>(p, head) : lov_aligned<RM_LABEL_U8>(p, head));
}

#define LOV_LAUNCH(LA, LB) label_overlap_kernel<LA, LB><<<grid, kRmThreads, 0, st>>>(a, b, head, nq, voxels, bins, cnt, badp)
#define LOV_DISPATCH_B(LA)                                  \
  do {                                                      \
    if (lt_b == RM_LABEL_F32) LOV_LAUNCH(LA, RM_LABEL_F32);      \
    else if (lt_b == RM_LABEL_I64) LOV_LAUNCH(LA, RM_LABEL_I64); \
    else LOV_LAUNCH(LA, RM_LABEL_U8);                         \
  } while (0)

static hipError_t launch_label_overlap(const void* a, int lt_a, const void* b, int lt_b, long long voxels, int bins, long long* counts,
                                       long long* bad, hipStream_t st) {
  unsigned long long* cnt = (unsigned long long*)counts;
  unsigned long long* badp = (unsigned long long*)bad;
  label_overlap_zero_kernel<<<(3 * bins + kRmThreads - 1) / kRmThreads, kRmThreads, 0, st>>>(cnt, 3 * bins, badp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the first `head` voxels (< 4) go one by one so that both volumes reach the alignment of their quads; when no head does that
  // (the two starts are skewed against each other) every voxel goes one by one
  long long head = 0, nq = 0;
  for (int h = 0; h < 4; ++h)
    if (lov_aligned_dyn(lt_a, a, h) && lov_aligned_dyn(lt_b, b, h)) {
      head = h < voxels ? h : voxels;
      nq = (voxels - head) / 4;
      break;
    }
  if (nq == 0) head = 0;
  const long long rest = voxels - 4 * nq, turns = (nq + kLovUnroll - 1) / kLovUnroll, units = turns > rest ? turns : rest;
  const long long need = (units + kRmThreads - 1) / kRmThreads;
  const int grid = (int)(need < kStreamMaxBlocks ? need : kStreamMaxBlocks);
  if (lt_a == RM_LABEL_F32) LOV_DISPATCH_B(RM_LABEL_F32);
  else if (lt_a == RM_LABEL_I64) LOV_DISPATCH_B(RM_LABEL_I64);
  else LOV_DISPATCH_B(RM_LABEL_U8);
  return hipGetLastError();
}

// ---- Jacobian determinant -----------------------------------------------------------------------------------------------------
// Running statistics of a set of determinants.  The log figures are kept as (count, mean, sum of squared deviations) and merged
// with the pairwise update of Chan, Golub & LeVeque, so that a constant field gives a deviation of exactly 0.
struct JacStats {
  double nonpos, npos, sum, mean, m2, mn, mx;
};
constexpr int kJacRec = 8;                 // doubles per slab record (7 used)

__device__ __forceinline__ JacStats jac_empty() { return {0.0, 0.0, 0.0, 0.0, 0.0, (double)INFINITY, -(double)INFINITY}; }
__device__ __forceinline__ JacStats jac_merge(const JacStats& a, const JacStats& b) {
  JacStats r;
  r.nonpos = a.nonpos + b.nonpos;
  r.sum = a.sum + b.sum;
  r.mn = fmin(a.mn, b.mn);
  r.mx = fmax(a.mx, b.mx);
  r.npos = a.npos + b.npos;
  if (b.npos == 0.0) {
    r.mean = a.mean, r.m2 = a.m2;
  } else if (a.npos == 0.0) {
    r.mean = b.mean, r.m2 = b.m2;
  } else {
    const double delta = b.mean - a.mean, fb = b.npos / r.npos;
    r.mean = a.mean + delta * fb;
    r.m2 = a.m2 + b.m2 + delta * delta * a.npos * fb;
  }
  return r;
}
__device__ __forceinline__ JacStats jac_shfl_down(const JacStats& s, int m) {
  JacStats r;
  r.nonpos = __shfl_down(s.nonpos, m, 64), r.npos = __shfl_down(s.npos, m, 64), r.sum = __shfl_down(s.sum, m, 64);
  r.mean = __shfl_down(s.mean, m, 64), r.m2 = __shfl_down(s.m2, m, 64), r.mn = __shfl_down(s.mn, m, 64), r.mx = __shfl_down(s.mx, m, 64);
  return r;
}
__device__ __forceinline__ void jac_store(double* __restrict__ p, const JacStats& s) {
  p[0] = s.nonpos, p[1] = s.npos, p[2] = s.sum, p[3] = s.mean, p[4] = s.m2, p[5] = s.mn, p[6] = s.mx;
}
__device__ __forceinline__ JacStats jac_load(const double* __restrict__ p) { return {p[0], p[1], p[2], p[3], p[4], p[5], p[6]}; }

// the workgroup's statistics in thread 0: lanes in a fixed tree, then the waves in order
__device__ __forceinline__ JacStats jac_block_merge(JacStats s, double* __restrict__ red) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) s = jac_merge(s, jac_shfl_down(s, m));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) jac_store(red + wave * kJacRec, s);
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s = jac_merge(s, jac_load(red + w * kJacRec));
  return s;
}

// VPT + 1 consecutive values of a row from element k0 on; the last one only where it exists (k0 + VPT < D)
template <int VPT>
__device__ __forceinline__ void jac_load_row(const float* __restrict__ p, int k0, int D, float (&v)[VPT + 1]) {
  if (VPT == 4) {
    const f32x4 q = *(const f32x4*)p;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = q[j];
  } else {
#pragma unroll
    for (int j = 0; j < VPT; ++j) v[j] = p[j];
  }
  v[VPT] = k0 + VPT < D ? p[VPT] : 0.f;
}

// A thread owns VPT consecutive determinants of one output row (i, j, k0 ..): it reads the rows (i, j), (i + 1, j), (i, j + 1) of
// the three channels.  VPT == 4 needs D % 4 == 0 and a 16-byte aligned field (every row quad is then aligned and inside its row).
template <int VPT, bool STATS>
__global__ __launch_bounds__(kRmThreads) void jacobian_det_kernel(const float* __restrict__ u, int H, int W, int D, int ident,
                                                                  float* __restrict__ jdet, double* __restrict__ part) {
  __shared__ double red[kRmWaves * kJacRec];
  const int Wo = W - 1, Do = D - 1, Dq = (Do + VPT - 1) / VPT;
  const long long V = (long long)H * W * D, plane = (long long)W * D, units = (long long)(H - 1) * Wo * Dq;
  const float one = ident ? 1.f : 0.f;
  unsigned nonpos = 0, npos = 0;
  float mn = INFINITY, mx = -INFINITY;
  double sum = 0.0, shift = 0.0, s1 = 0.0, s2 = 0.0;
  for (long long un = (long long)blockIdx.x * kRmThreads + threadIdx.x; un < units; un += (long long)gridDim.x * kRmThreads) {
    const int row = (int)(un / Dq), t = (int)(un - (long long)row * Dq), i = row / Wo, j = row - i * Wo, k0 = t * VPT;
    const long long base = ((long long)i * W + j) * D + k0;
    float c[3][VPT + 1], di[3][VPT + 1], dj[3][VPT + 1];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float* p = u + a * V + base;
      jac_load_row<VPT>(p, k0, D, c[a]);
      if (VPT == 4) {
        const f32x4 qi = *(const f32x4*)(p + plane), qj = *(const f32x4*)(p + D);
#pragma unroll
        for (int v = 0; v < 4; ++v) di[a][v] = qi[v], dj[a][v] = qj[v];
      } else {
#pragma unroll
        for (int v = 0; v < VPT; ++v) di[a][v] = p[plane + v], dj[a][v] = p[D + v];
      }
    }
    float det[VPT];
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
      float m[3][3];                      // m[b][A] = forward difference along axis A of component b of the map
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        m[b][0] = di[b][v] - c[b][v], m[b][1] = dj[b][v] - c[b][v], m[b][2] = c[b][v + 1] - c[b][v];
        m[b][b] += one;
      }
      det[v] = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
               m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    }
    if (jdet) {
      float* orow = jdet + ((long long)i * Wo + j) * Do + k0;
#pragma unroll
      for (int v = 0; v < VPT; ++v)
        if (k0 + v < Do) orow[v] = det[v];
    }
    if (STATS) {
#pragma unroll
      for (int v = 0; v < VPT; ++v) {
        if (k0 + v >= Do) continue;
        sum += (double)det[v];
        mn = fminf(mn, det[v]), mx = fmaxf(mx, det[v]);
        if (det[v] <= 0.f) ++nonpos;
        if (det[v] > 0.f) {
          const double lg = log((double)det[v]);
          if (npos == 0) shift = lg;      // the thread's first log: the sums below are of deviations from it
          ++npos;
          s1 += lg - shift, s2 += (lg - shift) * (lg - shift);
        }
      }
    }
  }
  if (!STATS) return;
  JacStats s = jac_empty();
  s.nonpos = (double)nonpos, s.npos = (double)npos, s.sum = sum, s.mn = (double)mn, s.mx = (double)mx;
  if (npos) {
    s.mean = shift + s1 / (double)npos;
    const double m2 = s2 - s1 * s1 / (double)npos;
    s.m2 = m2 > 0.0 ? m2 : 0.0;
  }
  s = jac_block_merge(s, red);
  if (threadIdx.x == 0) jac_store(part + (long long)blockIdx.x * kJacRec, s);
}

// one workgroup: thread t merges records t, t + 256, ... in order, then the workgroup's tree -> stats[6] =
// {share of determinants <= 0, min, max, mean, mean of log over the positive ones, population standard deviation of that log}
__global__ __launch_bounds__(kRmThreads) void jacobian_stats_finalize_kernel(const double* __restrict__ part, int nrec, double count,
                                                                             float* __restrict__ stats) {
  __shared__ double red[kRmWaves * kJacRec];
  JacStats s = jac_empty();
  for (int r = threadIdx.x; r < nrec; r += kRmThreads) s = jac_merge(s, jac_load(part + (long long)r * kJacRec));
  s = jac_block_merge(s, red);
  if (threadIdx.x == 0) {
    stats[0] = (float)(s.nonpos / count);
    stats[1] = (float)s.mn;
    stats[2] = (float)s.mx;
    stats[3] = (float)(s.sum / count);
    stats[4] = s.npos > 0.0 ? (float)s.mean : __int_as_float(0x7fc00000);
    stats[5] = s.npos > 1.0 ? (float)sqrt(s.m2 / s.npos) : 0.f;
  }
}

static inline int jac_vpt(const float* u, int D) { return (D % 4 == 0 && ((uintptr_t)u & 15) == 0) ? 4 : 1; }
static inline int jac_blocks(const float* u, int H, int W, int D) {
  const int vpt = jac_vpt(u, D);
  const long long units = (long long)(H - 1) * (W - 1) * ((D - 1 + vpt - 1) / vpt), need = (units + kRmThreads - 1) / kRmThreads;
  return (int)(need < kStreamMaxBlocks ? need : kStreamMaxBlocks);
}
static size_t jacobian_det_scratch_bytes(int H, int W, int D) {
  const long long need = ((long long)(H - 1) * (W - 1) * (D - 1) + kRmThreads - 1) / kRmThreads;       // covers both mappings
  return (size_t)(need < kStreamMaxBlocks ? need : kStreamMaxBlocks) * kJacRec * sizeof(double);
}

static hipError_t launch_jacobian_det(const float* disp, int H, int W, int D, int add_identity, float* jdet, float* stats, void* scratch,
                                      hipStream_t st) {
  const int grid = jac_blocks(disp, H, W, D), vec = jac_vpt(disp, D) == 4;
  double* part = (double*)scratch;
  if (stats) {
    if (vec) jacobian_det_kernel<4, true><<<grid, kRmThreads, 0, st>>>(disp, H, W, D, add_identity, jdet, part);
    else jacobian_det_kernel<1, true><<<grid, kRmThreads, 0, st>>>(disp, H, W, D, add_identity, jdet, part);
  } else {
    if (vec) jacobian_det_kernel<4, false><<<grid, kRmThreads, 0, st>>>(disp, H, W, D, add_identity, jdet, part);
    else jacobian_det_kernel<1, false><<<grid, kRmThreads, 0, st>>>(disp, H, W, D, add_identity, jdet, part);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !stats) return e;
  jacobian_stats_finalize_kernel<<<1, kRmThreads, 0, st>>>(part, grid, (double)(H - 1) * (W - 1) * (D - 1), stats);
  return hipGetLastError();
}

}  // namespace amx

namespace {
using amx::fail;

int lov_check_volume(const void* p, int dtype, const char* what) {
  if (!p) return fail(AMX_ERR_INVALID, "null %s", what);
  if (dtype < AMX_SEG_LABEL_F32 || dtype > AMX_SEG_LABEL_U8)
    return fail(AMX_ERR_INVALID, "%s dtype: AMX_SEG_LABEL_F32, _I64 or _U8 (got %d)", what, dtype);
  const uintptr_t need = dtype == AMX_SEG_LABEL_F32 ? 4 : (dtype == AMX_SEG_LABEL_I64 ? 8 : 1);
  if ((uintptr_t)p % need) return fail(AMX_ERR_INVALID, "%s is not aligned to its element size", what);
  return AMX_OK;
}
}  // namespace

extern "C" {

int amx_label_overlap(const void* d_a, int dtype_a, const void* d_b, int dtype_b, long long voxels, int bins, long long* d_counts,
                      long long* d_bad, void* stream) {
  if (int rc = lov_check_volume(d_a, dtype_a, "d_a")) return rc;
  if (int rc = lov_check_volume(d_b, dtype_b, "d_b")) return rc;
  if (!d_counts || !d_bad || (uintptr_t)d_counts % 8 || (uintptr_t)d_bad % 8) return fail(AMX_ERR_INVALID, "null or unaligned output");
  if (bins < 1 || bins > amx::kLovMaxBins) return fail(AMX_ERR_INVALID, "1 <= bins <= %d (got %d)", amx::kLovMaxBins, bins);
  if (voxels < 1 || voxels >= (1LL << 40)) return fail(AMX_ERR_SHAPE, "1 <= voxels < 2^40 (got %lld)", voxels);
  AMX_HIP(amx::launch_label_overlap(d_a, dtype_a, d_b, dtype_b, voxels, bins, d_counts, d_bad, (hipStream_t)stream));
  return AMX_OK;
}

size_t amx_jacobian_det_scratch_bytes(int H, int W, int D) {
  if (H < 2 || W < 2 || D < 2 || (long long)H * W * D >= (1LL << 31)) return 0;
  return amx::jacobian_det_scratch_bytes(H, W, D);
}

int amx_jacobian_det(const float* d_disp, int H, int W, int D, int add_identity, float* d_jdet, float* d_stats, void* d_scratch,
                     size_t scratch_bytes, void* stream) {
  if (!d_disp || (uintptr_t)d_disp % 4) return fail(AMX_ERR_INVALID, "null or unaligned d_disp");
  if (H < 2 || W < 2 || D < 2) return fail(AMX_ERR_INVALID, "H, W, D >= 2 (got %d, %d, %d)", H, W, D);
  if ((long long)H * W * D >= (1LL << 31)) return fail(AMX_ERR_SHAPE, "volume < 2^31 voxels (got %d, %d, %d)", H, W, D);
  if (!d_jdet && !d_stats) return fail(AMX_ERR_INVALID, "d_jdet and d_stats are both null");
  if ((uintptr_t)d_jdet % 4 || (uintptr_t)d_stats % 4) return fail(AMX_ERR_INVALID, "unaligned output");
  if (d_jdet) {
    const uintptr_t j0 = (uintptr_t)d_jdet, j1 = j0 + (size_t)(H - 1) * (W - 1) * (D - 1) * sizeof(float);
    const uintptr_t u0 = (uintptr_t)d_disp, u1 = u0 + (size_t)3 * H * W * D * sizeof(float);
    if (j0 < u1 && u0 < j1) return fail(AMX_ERR_INVALID, "d_jdet overlaps d_disp");
  }
  if (d_stats) {
    const size_t need = amx::jacobian_det_scratch_bytes(H, W, D);
    if (!d_scratch || (uintptr_t)d_scratch % 8 || scratch_bytes < need)
      return fail(AMX_ERR_INVALID, "the statistics need %zu bytes of 8-byte aligned scratch (got %zu)", need, scratch_bytes);
  }
  AMX_HIP(amx::launch_jacobian_det(d_disp, H, W, D, add_identity != 0, d_jdet, d_stats, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

}  // extern "C"
