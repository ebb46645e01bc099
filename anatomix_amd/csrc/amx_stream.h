// anatomix_amd -- what the streaming units (amx_segloss.hip, amx_segaug.hip, amx_preaug.hip, amx_synth.hip, amx_labels.hip, amx_regmetrics.hip,
// amx_reginstopt.hip) share: the four-voxel tile access, the ascending xor butterfly over a wave and the LDS tree sum over a
// workgroup, and for the three augmentation units the volume dims, the workgroup min / max with its partial slab, the
// degree-3 polynomial sum and the centred taps.  Each reduction here has ONE order; a reduction in another order
// (amx_mlp.hip's wave_sum, amx_supcon.hip's block_sum, ...) is another function and stays in its unit, since merging them would
// change results in the last bit.
#pragma once
#include <stdint.h>

#include "amx_common.h"

namespace amx {

constexpr int kStreamMaxBlocks = 2048;     // workgroups of a streaming launch (8 per CU): bounds the partial slabs

// ---- streaming tile ---------------------------------------------------------------------------------------------------------
// A workgroup of THREADS threads covers tile t = VPT * THREADS voxels of a row of V, a thread owning VPT of them: VPT consecutive
// voxels behind one 16-byte access (VEC: V % 4 == 0 and aligned bases, so a quad is inside the row or outside it as a whole),
// otherwise VPT voxels THREADS apart accessed one by one (coalesced across lanes).
template <int THREADS = 256, int VPT = 4>
struct StreamTile {
  static_assert(VPT == 4, "the vector path is one 16-byte access of four floats");
  static constexpr int kThreads = THREADS, kWaves = THREADS / 64, kVpt = VPT, kTile = THREADS * VPT;

  // voxel j of this thread in tile t
  template <bool VEC>
  static __device__ __forceinline__ long long voxel(int t, int j) {
    return VEC ? (long long)t * kTile + threadIdx.x * VPT + j : (long long)t * kTile + j * THREADS + threadIdx.x;
  }

  // voxels past V read as 0
  template <bool VEC>
  static __device__ __forceinline__ void load4(const float* __restrict__ row, int t, long long V, float (&v)[VPT]) {
    if (VEC) {
      const long long o = voxel<true>(t, 0);
      f32x4 q = {0.f, 0.f, 0.f, 0.f};
      if (o < V) q = *(const f32x4*)(row + o);
#pragma unroll
      for (int j = 0; j < VPT; ++j) v[j] = q[j];
    } else {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const long long o = voxel<false>(t, j);
        v[j] = o < V ? row[o] : 0.f;
      }
    }
  }

  // uint8 voxels (labels) as ints; VEC: one 4-byte load (a 4-byte aligned base)
  template <bool VEC>
  static __device__ __forceinline__ void load4(const unsigned char* __restrict__ row, int t, long long V, int (&l)[VPT]) {
    if (VEC) {
      const long long o = voxel<true>(t, 0);
      uchar4 q = make_uchar4(0, 0, 0, 0);
      if (o < V) q = *(const uchar4*)(row + o);
      l[0] = q.x, l[1] = q.y, l[2] = q.z, l[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const long long o = voxel<false>(t, j);
        l[j] = o < V ? row[o] : 0;
      }
    }
  }

  template <bool VEC>
  static __device__ __forceinline__ void store4(float* __restrict__ row, int t, long long V, const float (&v)[VPT]) {
    if (VEC) {
      const long long o = voxel<true>(t, 0);
      if (o < V) *(f32x4*)(row + o) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const long long o = voxel<false>(t, j);
        if (o < V) row[o] = v[j];
      }
    }
  }

  // VEC: one 4-byte store (a 4-byte aligned base)
  template <bool VEC>
  static __device__ __forceinline__ void store4(unsigned char* __restrict__ row, int t, long long V, const unsigned char (&v)[VPT]) {
    if (VEC) {
      const long long o = voxel<true>(t, 0);
      if (o < V) *(uchar4*)(row + o) = make_uchar4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const long long o = voxel<false>(t, j);
        if (o < V) row[o] = v[j];
      }
    }
  }

  // host side: tiles of a row, and the grid.x of a launch over n rows (grid.y): all the tiles, or the share of the cap
  static inline long long tiles(long long V) { return (V + kTile - 1) / kTile; }
  static inline int chunks(int n, long long V) {
    const long long cap = kStreamMaxBlocks / n > 1 ? kStreamMaxBlocks / n : 1, t = tiles(V);
    return (int)(t < cap ? t : cap);
  }
};

// ---- volume dims ------------------------------------------------------------------------------------------------------------
// a [d][h][w] volume streamed as one row of V voxels in ntiles tiles (the base of a kernel argument that needs more: SynApp)
struct StreamDims {
  int d, h, w;
  long long V;
  int ntiles;

  static inline StreamDims make(int d, int h, int w) {
    StreamDims g;
    g.d = d, g.h = h, g.w = w, g.V = (long long)d * h * w, g.ntiles = (int)StreamTile<>::tiles(g.V);
    return g;
  }
  // (z, y, x) of voxel o
  __device__ __forceinline__ void split(long long o, int& z, int& y, int& x) const {
    x = (int)(o % w), y = (int)((o / w) % h), z = (int)(o / ((long long)w * h));
  }
};

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// ---- butterfly reduce -------------------------------------------------------------------------------------------------------
struct SumOp {
  template <typename T>
  static __device__ __forceinline__ T apply(T a, T b) { return a + b; }
};
struct MinOp {
  static __device__ __forceinline__ float apply(float a, float b) { return fminf(a, b); }
  static __device__ __forceinline__ double apply(double a, double b) { return fmin(a, b); }
  static __device__ __forceinline__ int apply(int a, int b) { return a < b ? a : b; }
};
struct MaxOp {
  static __device__ __forceinline__ float apply(float a, float b) { return fmaxf(a, b); }
  static __device__ __forceinline__ double apply(double a, double b) { return fmax(a, b); }
  static __device__ __forceinline__ int apply(int a, int b) { return a > b ? a : b; }
};

// Op over the 64 lanes of a wave, partner masks 1, 2, 4, 8, 16, 32 in that order; every lane gets the result
template <typename Op, typename T>
__device__ __forceinline__ T wave_reduce_xor(T v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = Op::apply(v, __shfl_xor(v, m, 64));
  return v;
}

// ---- minimum and maximum ----------------------------------------------------------------------------------------------------
// {lo, hi} of the workgroup (a StreamTile<> one: four waves) -> dst[2]: per thread, wave (shuffles), workgroup (LDS).  Every
// workgroup writes its pair, with (+inf, -inf) when it saw no value.
__device__ __forceinline__ void block_minmax(float lo, float hi, float* __restrict__ dst) {
  static_assert(StreamTile<>::kWaves == 4, "the last step combines four waves");
  __shared__ float red[StreamTile<>::kWaves][2];
  lo = wave_reduce_xor<MinOp>(lo);
  hi = wave_reduce_xor<MaxOp>(hi);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) red[wave][0] = lo, red[wave][1] = hi;
  __syncthreads();
  if (threadIdx.x == 0) {
    dst[0] = fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0]));
    dst[1] = fmaxf(fmaxf(red[0][1], red[1][1]), fmaxf(red[2][1], red[3][1]));
  }
}
// the slab pair of this workgroup of a (chunks, rows) grid: pair [row][chunk], what the finalize kernel of amx_segaug.hip reads
__device__ __forceinline__ float* minmax_slab(float* __restrict__ part) { return part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2; }

// ---- trilinear upsample ------------------------------------------------------------------------------------------------------
// torch's source index of the trilinear upsample (align_corners=False) of output voxel o of an axis with cn coarse points and
// rs = 1 / scale: neighbours i0, i1 (the upper one clamped) and the weight of i1
__device__ __forceinline__ void trilinear_src(int o, float rs, int cn, int& i0, int& i1, float& l1) {
  const float src = fmaxf(rs * ((float)o + 0.5f) - 0.5f, 0.f);
  i0 = min((int)src, cn - 1);
  i1 = min(i0 + 1, cn - 1);
  l1 = src - (float)i0;
}

// ---- bias field and taps ----------------------------------------------------------------------------------------------------
// coordinate i of linspace(-1, 1, n)
__device__ __forceinline__ float lin_coord(int i, int n) { return n > 1 ? -1.f + 2.f * (float)i / (float)(n - 1) : -1.f; }

// sum of c[q] pz[i] py[j] px[k] over i + j + k <= 3, (i, j, k) lexicographic: the 20 terms in that order
__device__ __forceinline__ float poly3_sum(const float (&c)[20], const float (&pz)[4], const float (&py)[4], const float (&px)[4]) {
  float f = 0.f;
  int q = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4 - i; ++j)
#pragma unroll
      for (int k = 0; k < 4 - i - j; ++k) f += c[q++] * (pz[i] * py[j] * px[k]);
  return f;
}

// the 2 r + 1 taps of one axis (r <= R) centred in registers: tap[k + R], 0 outside the radius, so that an unrolled loop over
// -R .. R indexes registers statically (uniform, so scalar loads)
template <int R>
__device__ __forceinline__ void load_centred_taps(const float* __restrict__ taps, int r, float (&tap)[2 * R + 1]) {
#pragma unroll
  for (int k = -R; k <= R; ++k) tap[k + R] = (k >= -r && k <= r) ? taps[k + r] : 0.f;
}

// ---- tree sum ---------------------------------------------------------------------------------------------------------------
// fixed-order sum of one value per thread over the NT threads of a workgroup through red[NT] (LDS): halving tree, every thread
// gets the result.  The trailing barrier frees red for the next call (and orders the caller's earlier stores like any barrier).
template <typename T, int NT>
__device__ __forceinline__ T block_tree_sum(T v, T* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const T r = red[0];
  __syncthreads();
  return r;
}

}  // namespace amx
