// anatomix_amd -- step 1 of the reference's synthetic data generation (synthetic-data-generation/step1_generate_labels.py with
// datagen_utils.py:26-447) on a batch of label ensembles, uint8 [batch][d][h][w]:
//   compose        per voxel the last template with a non-zero nearest-neighbour sample under its affine map (float64 coordinates,
//                  scipy's order=0 / 'grid-wrap'), the padded template never materialised; scans from the last template down
//   median         exact 3 x 3 x 3 median with border replication: an LDS tile with a one-voxel halo, two voxels per thread as the
//                  16-bit halves of a register, a forgetful min / max selection network on v_pk_min_u16 / v_pk_max_u16
//   sphere mask    the deformed sphere in one kernel: three trilinear upsamples per component, torch's grid_sample coordinate
//                  arithmetic (un-normalise, reflect, clip, round half to even), an integer distance test; no field is stored
//   apply mask     label = mask ? label + 1 : 0 with the maximum label as per-workgroup partials and a finalize
//   envelope       dilate & ~erode with a ball of radius 2 .. 4 under scipy's `reflect`: rows packed as 64-bit words in LDS, the
//                  ball as a union of x-runs (shifts and ORs), erosion as ~dilate(~mask)
// One launch per stage with the ensemble on a grid axis; what differs per ensemble is read from a device table of
// amx_labels_ensemble records.  Integer arithmetic, and float arithmetic in one fixed order: two runs agree bit for bit.
#include <math.h>
#include <stdio.h>

#include "amx_device.h"
#include "amx_launch.h"
#include "amx_stream.h"

namespace amx {

using Lab = StreamTile<>;
using LabTpl = amx_labels_template;
using LabEns = amx_labels_ensemble;

// ---- compose -----------------------------------------------------------------------------------------------------------------
// sample of template T at output voxel (o0, o1, o2): products and sums rounded one by one (no contraction), as numpy and scipy do
__device__ __forceinline__ bool lab_sample(const LabTpl& T, const unsigned char* __restrict__ bytes, double o0, double o1, double o2) {
#pragma clang fp contract(off)
  long long idx = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double* m = T.affine + 4 * a;
    const double x = ((m[3] + o0 * m[0]) + o1 * m[1]) + o2 * m[2];
    const int i = (int)floor(x + 0.5);      // |x| < 1e9: the launcher checks the map's reach
    int r = i % T.padded[a];
    if (r < 0) r += T.padded[a];
    r -= T.before[a];
    if (r < 0 || r >= T.crop[a]) return false;
    idx = idx * T.crop[a] + r;
  }
  return bytes[T.offset + idx] != 0;
}

template <bool VEC>
__global__ __launch_bounds__(Lab::kThreads) void lab_compose_kernel(StreamDims g, const unsigned char* __restrict__ bytes,
                                                                   const LabTpl* __restrict__ templates, const LabEns* __restrict__ table,
                                                                   unsigned char* __restrict__ out) {
  const int b = blockIdx.y;
  const LabEns e = table[b];
  const LabTpl* tt = templates + e.first;
  unsigned char* dst = out + (long long)b * g.V;
  for (int t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    unsigned char q[Lab::kVpt];
#pragma unroll
    for (int j = 0; j < Lab::kVpt; ++j) {
      const long long o = Lab::voxel<VEC>(t, j);
      q[j] = 0;
      if (o >= g.V) continue;
      int z, y, x;
      g.split(o, z, y, x);
      // template 0 writes label 0: the scan stops above it
      for (int k = e.count - 1; k >= 1; --k)
        if (lab_sample(tt[k], bytes, (double)z, (double)y, (double)x)) {
          q[j] = (unsigned char)k;
          break;
        }
    }
    Lab::store4<VEC>(dst, t, g.V, q);
  }
}

// ---- median ------------------------------------------------------------------------------------------------------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
constexpr int kMedX = 32, kMedY = 8, kMedZ = 4;                       // outputs of a workgroup
constexpr int kMedRow = 36, kMedHy = kMedY + 2, kMedHz = kMedZ + 2;   // halo tile: rows of 34 bytes, padded to 36

__device__ __forceinline__ void med_exchange(u16x2& lo, u16x2& hi) {
  const u16x2 a = __builtin_elementwise_min(lo, hi), b = __builtin_elementwise_max(lo, hi);
  lo = a, hi = b;
}

// The median of 27: of any 15 values neither the smallest nor the largest can be the median (14 values lie on its other side),
// so both are dropped and the next value joins, 15, 14, ... 3 values; the middle of the last three is element 13 of the sorted
// 27.  All indices are compile-time constants after unrolling, so v stays in registers.
__device__ __forceinline__ u16x2 med27(u16x2 (&v)[27]) {
  // the window is v[15 - n .. 14]; a step moves its minimum to the front and its maximum to v[14], the front is dropped by the
  // next step's window and the next input, v[30 - n], takes the maximum's place
#pragma unroll
  for (int n = 15; n >= 3; --n) {
    const int lo = 15 - n, hi = 14, half = (n + 1) / 2;
#pragma unroll
    for (int i = 0; i < n / 2; ++i) med_exchange(v[lo + i], v[hi - i]);
#pragma unroll
    for (int i = 1; i < half; ++i) med_exchange(v[lo], v[lo + i]);
#pragma unroll
    for (int i = hi - half + 1; i < hi; ++i) med_exchange(v[i], v[hi]);
    if (n > 3) v[hi] = v[30 - n];
  }
  return v[13];
}

__global__ __launch_bounds__(256) void lab_median_kernel(int d, int h, int w, int tiles_y, int require, const unsigned char* __restrict__ in,
                                                         unsigned char* __restrict__ out, const LabEns* __restrict__ table) {
  __shared__ unsigned char tile[kMedHz * kMedHy * kMedRow];
  const int b = blockIdx.z;
  const long long V = (long long)d * h * w;
  const unsigned char* src = in + (long long)b * V;
  unsigned char* dst = out + (long long)b * V;
  const int x0 = blockIdx.x * kMedX, y0 = (blockIdx.y % tiles_y) * kMedY, z0 = (blockIdx.y / tiles_y) * kMedZ;
  const bool on = (table[b].flags & require) == require;
  const int lx = (threadIdx.x & 15) * 2, ly = (threadIdx.x >> 4) & 7, lz = threadIdx.x >> 7;
  if (on) {
    for (int e = threadIdx.x; e < kMedHz * kMedHy * (kMedX + 2); e += 256) {
      const int hx = e % (kMedX + 2), hy = (e / (kMedX + 2)) % kMedHy, hz = e / ((kMedX + 2) * kMedHy);
      const int sx = min(max(x0 + hx - 1, 0), w - 1), sy = min(max(y0 + hy - 1, 0), h - 1), sz = min(max(z0 + hz - 1, 0), d - 1);
      tile[(hz * kMedHy + hy) * kMedRow + hx] = src[((long long)sz * h + sy) * w + sx];
    }
    __syncthreads();
  }
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int z = z0 + lz + 2 * pass, y = y0 + ly, x = x0 + lx;
    if (z >= d || y >= h || x >= w) continue;
    const long long o = ((long long)z * h + y) * w + x;
    if (!on) {
      dst[o] = src[o];
      if (x + 1 < w) dst[o + 1] = src[o + 1];
      continue;
    }
    u16x2 v[27];
#pragma unroll
    for (int dz = 0; dz < 3; ++dz)
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const unsigned char* r = tile + ((lz + 2 * pass + dz) * kMedHy + ly + dy) * kMedRow + lx;
        const unsigned short b0 = r[0], b1 = r[1], b2 = r[2], b3 = r[3];
        u16x2* q = v + (dz * 3 + dy) * 3;
        q[0] = u16x2{b0, b1}, q[1] = u16x2{b1, b2}, q[2] = u16x2{b2, b3};
      }
    const u16x2 m = med27(v);
    dst[o] = (unsigned char)m[0];
    if (x + 1 < w) dst[o + 1] = (unsigned char)m[1];
  }
}

// ---- deformed-sphere mask ----------------------------------------------------------------------------------------------------
struct LabSphere {
  int size;
  float rs[3];             // 1 / scale
  const float* grid[3];    // [batch][3][cn][cn][cn], cn = 16, 8, 4
};

// trilinear upsample (align_corners=False) of one coarse grid [cn]^3 at voxel (z, y, x), in torch's order of blends, every product
// and sum of the blends rounded.  The source index, trilinear_src, is shared with amx_synth.hip and may contract its one
// multiply-subtract as it does there, so the blend weight is pinned to torch's only up to that last bit; the 1e-4 margin of the
// tests covers it
__device__ __forceinline__ float lab_upsample(const float* __restrict__ g, int cn, float rs, int z, int y, int x) {
#pragma clang fp contract(off)
  int z0, z1, y0, y1, x0, x1;
  float lz, ly, lx;
  trilinear_src(z, rs, cn, z0, z1, lz);
  trilinear_src(y, rs, cn, y0, y1, ly);
  trilinear_src(x, rs, cn, x0, x1, lx);
  const float* p00 = g + (z0 * cn + y0) * cn;
  const float* p01 = g + (z0 * cn + y1) * cn;
  const float* p10 = g + (z1 * cn + y0) * cn;
  const float* p11 = g + (z1 * cn + y1) * cn;
  const float kx = 1.f - lx, ky = 1.f - ly, kz = 1.f - lz;
  return kz * (ky * (kx * p00[x0] + lx * p00[x1]) + ly * (kx * p01[x0] + lx * p01[x1])) +
         lz * (ky * (kx * p10[x0] + lx * p10[x1]) + ly * (kx * p11[x0] + lx * p11[x1]));
}

// the normalised coordinate of grid component `at` displaced by disp voxels, as the reference forms it in float32
__device__ __forceinline__ float lab_normalised(int at, float disp, double half, double span) {
#pragma clang fp contract(off)
  const float base = (float)(2.0 * ((double)at - half) / span);      // the float64 grid unit rounded to float32
  return base + (2.f * disp) / (float)span;
}

// torch's grid_sample(mode='nearest', padding_mode='reflection', align_corners=False) source voxel of normalised coordinate g
__device__ __forceinline__ int lab_nearest_reflect(float g, int size) {
#pragma clang fp contract(off)
  const float n = (float)size;
  float x = ((g + 1.f) * n - 1.f) / 2.f;
  // reflect about [-0.5, size - 0.5]
  const float in = fabsf(x + 0.5f), extra = fmodf(in, n);
  const int flips = (int)floorf(in / n);
  x = (flips & 1) ? (n - extra) - 0.5f : extra - 0.5f;
  x = fminf(n - 1.f, fmaxf(x, 0.f));
  return (int)rintf(x);
}

template <bool VEC>
__global__ __launch_bounds__(Lab::kThreads) void lab_sphere_kernel(LabSphere a, StreamDims g, unsigned char* __restrict__ mask,
                                                                  const LabEns* __restrict__ table) {
  const int b = blockIdx.y;
  const LabEns e = table[b];
  if (!(e.flags & AMX_LABELS_MASK)) return;
  unsigned char* dst = mask + (long long)b * g.V;
  const int S = a.size, c = S / 2;
  const double half = (double)(S - 1) / 2.0, span = (double)(S - 1);
  const int r2 = e.radius * e.radius;
  for (int t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    unsigned char q[Lab::kVpt];
#pragma unroll
    for (int j = 0; j < Lab::kVpt; ++j) {
      const long long o = Lab::voxel<VEC>(t, j);
      q[j] = 0;
      if (o >= g.V) continue;
      int pos[3];      // pos[0] = w index, pos[1] = h, pos[2] = d: the axis component c of the grid addresses
      g.split(o, pos[2], pos[1], pos[0]);
      int dist = 0;
#pragma unroll
      for (int comp = 0; comp < 3; ++comp) {
        float disp = 0.f;
        int cn = 16;
#pragma unroll
        for (int s = 0; s < 3; ++s, cn >>= 1)
          disp += lab_upsample(a.grid[s] + ((long long)b * 3 + comp) * cn * cn * cn, cn, a.rs[s], pos[2], pos[1], pos[0]);
        const int qv = lab_nearest_reflect(lab_normalised(pos[comp], disp, half, span), S), dq = qv - (c + e.shift[2 - comp]);
        dist += dq * dq;
      }
      q[j] = dist <= r2 ? 1 : 0;
    }
    Lab::store4<VEC>(dst, t, g.V, q);
  }
}

// ---- apply mask ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lab_block_max(int v) {
  static_assert(Lab::kWaves == 4, "the last step combines four waves");
  __shared__ int red[Lab::kWaves];
  v = wave_reduce_xor<MaxOp>(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return max(max(red[0], red[1]), max(red[2], red[3]));
}

template <bool VEC>
__global__ __launch_bounds__(Lab::kThreads) void lab_apply_kernel(unsigned char* __restrict__ labels, const unsigned char* __restrict__ mask,
                                                                 long long V, int ntiles, const LabEns* __restrict__ table, int* __restrict__ part) {
  const int b = blockIdx.y;
  const bool on = table[b].flags & AMX_LABELS_MASK;
  unsigned char* lab = labels + (long long)b * V;
  const unsigned char* m = mask + (long long)b * V;
  int hi = 0;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    int l[Lab::kVpt];
    Lab::load4<VEC>(lab, t, V, l);
    if (on) {
      int k[Lab::kVpt];
      unsigned char q[Lab::kVpt];
      Lab::load4<VEC>(m, t, V, k);
#pragma unroll
      for (int j = 0; j < Lab::kVpt; ++j) l[j] = k[j] ? l[j] + 1 : 0, q[j] = (unsigned char)l[j];
      Lab::store4<VEC>(lab, t, V, q);
    }
#pragma unroll
    for (int j = 0; j < Lab::kVpt; ++j) hi = max(hi, l[j]);      // voxels past V read as 0
  }
  hi = lab_block_max(hi);
  if (threadIdx.x == 0) part[(long long)b * gridDim.x + blockIdx.x] = hi;
}

// grid (batch): the maximum over an ensemble's nchunk partials
__global__ __launch_bounds__(Lab::kThreads) void lab_max_finalize_kernel(const int* __restrict__ part, int nchunk, int* __restrict__ out) {
  int hi = 0;
  for (int c = threadIdx.x; c < nchunk; c += Lab::kThreads) hi = max(hi, part[(long long)blockIdx.x * nchunk + c]);
  hi = lab_block_max(hi);
  if (threadIdx.x == 0) out[blockIdx.x] = hi;
}

// ---- envelope ------------------------------------------------------------------------------------------------------------------
constexpr int kEnvR = 4, kEnvX = 64 - 2 * kEnvR, kEnvY = 16, kEnvZ = 16;      // 56 outputs per 64-bit row, 16 x 16 rows per workgroup
constexpr int kEnvHy = kEnvY + 2 * kEnvR, kEnvHz = kEnvZ + 2 * kEnvR;

// scipy's `reflect` (the edge voxel repeated), then clamped: one reflection covers every index a valid output reads
__device__ __forceinline__ int lab_reflect(int i, int n) {
  i = i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i);
  return min(max(i, 0), n - 1);
}

// OR of the row shifted by -hw .. hw
__device__ __forceinline__ unsigned long long lab_run_or(unsigned long long w, int hw) {
  unsigned long long acc = w;
  for (int k = 1; k <= hw; ++k) acc |= (w << k) | (w >> k);
  return acc;
}

__global__ __launch_bounds__(256) void lab_envelope_kernel(int d, int h, int w, int tiles_y, unsigned char* __restrict__ labels,
                                                           const unsigned char* __restrict__ mask, const int* __restrict__ max_label,
                                                           const LabEns* __restrict__ table) {
  __shared__ unsigned long long rows[kEnvHz * kEnvHy];
  const int b = blockIdx.z;
  const LabEns e = table[b];
  if (!(e.flags & AMX_LABELS_ENVELOPE)) return;
  const long long V = (long long)d * h * w;
  const unsigned char* m = mask + (long long)b * V;
  unsigned char* lab = labels + (long long)b * V;
  const int x0 = blockIdx.x * kEnvX, y0 = (blockIdx.y % tiles_y) * kEnvY, z0 = (blockIdx.y / tiles_y) * kEnvZ;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // a wave packs one halo row per step: bit l of the word is the mask at x0 - 4 + l
  const int sx = lab_reflect(x0 - kEnvR + lane, w);
  for (int r = wave; r < kEnvHz * kEnvHy; r += 4) {
    const int hy = r % kEnvHy, hz = r / kEnvHy;
    const int sy = lab_reflect(y0 - kEnvR + hy, h), sz = lab_reflect(z0 - kEnvR + hz, d);
    const unsigned long long bits = __ballot(m[((long long)sz * h + sy) * w + sx] != 0);
    if (lane == 0) rows[r] = bits;
  }
  __syncthreads();
  const int ty = threadIdx.x & 15, tz = threadIdx.x >> 4, y = y0 + ty, z = z0 + tz;
  if (y >= h || z >= d) return;
  const int rad = e.ball, rad2 = rad * rad;
  unsigned long long dil = 0, dil_not = 0;
  for (int dz = -rad; dz <= rad; ++dz)
    for (int dy = -rad; dy <= rad; ++dy) {
      const int rem = rad2 - dz * dz - dy * dy;
      if (rem < 0) continue;
      int hw = 0;
      while ((hw + 1) * (hw + 1) <= rem) ++hw;
      const unsigned long long row = rows[(tz + kEnvR + dz) * kEnvHy + ty + kEnvR + dy];
      dil |= lab_run_or(row, hw);
      dil_not |= lab_run_or(~row, hw);
    }
  // erode = ~dilate(~mask): the envelope dilate & ~erode is where both dilations are set
  unsigned long long env = (dil & dil_not) >> kEnvR;
  const int nx = min(kEnvX, w - x0);
  if (nx < 64) env &= (1ull << nx) - 1;
  const unsigned char value = (unsigned char)(1 + max_label[b]);
  unsigned char* dst = lab + ((long long)z * h + y) * w + x0;
  while (env) {
    const int j = __ffsll((long long)env) - 1;
    dst[j] = value;
    env &= env - 1;
  }
}

// ---- step 0: merge of a segmentation folder ----------------------------------------------------------------------------------
// One pass over a batch of n mask rows: the sum of every row (its emptiness test) and the two merged rows (ribs, vertebrae).  A
// lane owns 16 consecutive voxels of every row per step; the merged voxels sit in registers as 16-bit halves (even bytes in one
// word, odd bytes in the other), which hold 256 rows of 255 plus an accumulated 255 without a carry.
struct LabMerge {
  unsigned char group[AMX_LABELS_MAX_MERGE];      // kernel argument: read through scalar loads
};
typedef __attribute__((ext_vector_type(4))) unsigned lab_u32x4;
constexpr int kMergeInFlight = 4;

__device__ __forceinline__ unsigned lab_byte_sum(unsigned w) { return __builtin_amdgcn_sad_u8(w, 0u, 0u); }

// adds v, which only the lanes of a wave's file share hold, into the block's slot: the wave's sum by lane 0
__device__ __forceinline__ void lab_wave_add(unsigned long long* slot, unsigned v) {
  v = wave_reduce_xor<SumOp>(v);
  if ((threadIdx.x & 63) == 0) atomicAdd(slot, (unsigned long long)v);
}

// 16-bit halves of a merged quad -> bytes clamped to 255; `over` is set when a half passed 255
__device__ __forceinline__ unsigned lab_pack_clamped(unsigned even, unsigned odd, bool& over) {
  over |= ((even | odd) & 0xff00ff00u) != 0;
  const unsigned e0 = min(even & 0xffffu, 255u), e1 = min(even >> 16, 255u), o0 = min(odd & 0xffffu, 255u), o1 = min(odd >> 16, 255u);
  return e0 | (o0 << 8) | (e1 << 16) | (o1 << 24);
}

__global__ __launch_bounds__(256) void lab_merge_kernel(LabMerge a, const unsigned char* __restrict__ masks, int n, long long voxels,
                                                        long long stride, unsigned char* __restrict__ merged,
                                                        unsigned long long* __restrict__ sums, int* __restrict__ overflow, int accumulate) {
  __shared__ unsigned long long part[AMX_LABELS_MAX_MERGE + 2];
  for (int i = threadIdx.x; i < n + 2; i += 256) part[i] = 0;
  __syncthreads();
  const long long nvec = voxels >> 4;
  unsigned long long msum[2] = {0, 0};
  bool over[2] = {false, false};
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v - threadIdx.x < nvec; v += (long long)gridDim.x * 256) {
    // (the loop bound is uniform over the workgroup, so that every wave takes part in the shuffles below; lanes past nvec hold zeros)
    const bool live = v < nvec;
    unsigned even[2][4], odd[2][4];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      lab_u32x4 q = {0u, 0u, 0u, 0u};
      if (accumulate && live) q = *(const lab_u32x4*)(merged + g * stride + v * 16);
#pragma unroll
      for (int j = 0; j < 4; ++j) even[g][j] = q[j] & 0x00ff00ffu, odd[g][j] = (q[j] >> 8) & 0x00ff00ffu;
    }
    for (int f0 = 0; f0 < n; f0 += kMergeInFlight) {
      lab_u32x4 qs[kMergeInFlight];      // the loads of kMergeInFlight files are issued before the first is used
#pragma unroll
      for (int k = 0; k < kMergeInFlight; ++k) {
        qs[k] = lab_u32x4{0u, 0u, 0u, 0u};
        if (live && f0 + k < n) qs[k] = *(const lab_u32x4*)(masks + (f0 + k) * stride + v * 16);
      }
#pragma unroll
      for (int k = 0; k < kMergeInFlight; ++k) {
        const lab_u32x4 q = qs[k];
        const int f = f0 + k;
        const unsigned s = lab_byte_sum(q[0]) + lab_byte_sum(q[1]) + lab_byte_sum(q[2]) + lab_byte_sum(q[3]);
        if (__ballot(s != 0) == 0) continue;      // wave-uniform: most of a mask is background (and files past n read as zeros)
        lab_wave_add(part + f, s);
        const int grp = a.group[f];
        if (grp == 0) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned e = q[j] & 0x00ff00ffu, o = (q[j] >> 8) & 0x00ff00ffu;
          if (grp == 1) even[0][j] += e, odd[0][j] += o;
          else even[1][j] += e, odd[1][j] += o;
        }
      }
    }
    if (live) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        lab_u32x4 q;
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = lab_pack_clamped(even[g][j], odd[g][j], over[g]), msum[g] += lab_byte_sum(q[j]);
        *(lab_u32x4*)(merged + g * stride + v * 16) = q;
      }
    }
  }
  // the voxels % 16 tail: one voxel per lane of the first wave of workgroup 0
  const int tail = (int)(voxels & 15);
  if (blockIdx.x == 0 && threadIdx.x < 64 && tail) {
    const bool live = (int)threadIdx.x < tail;
    const long long o = (nvec << 4) + threadIdx.x;
    unsigned acc[2] = {0, 0};
    if (accumulate && live) acc[0] = merged[o], acc[1] = merged[stride + o];
    for (int f = 0; f < n; ++f) {
      const unsigned s = live ? masks[f * stride + o] : 0u;
      if (__ballot(s != 0) == 0) continue;
      lab_wave_add(part + f, s);
      const int grp = a.group[f];
      if (grp) acc[grp - 1] += s;
    }
    if (live) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        over[g] |= acc[g] > 255u;
        acc[g] = min(acc[g], 255u);
        msum[g] += acc[g];
        merged[g * stride + o] = (unsigned char)acc[g];
      }
    }
  }
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const unsigned long long m = wave_reduce_xor<SumOp>(msum[g]);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(part + n + g, m);
    if (over[g]) overflow[g] = 1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n + 2; i += 256)
    if (part[i]) atomicAdd(sums + i, part[i]);
}

}  // namespace amx

namespace {
using amx::fail;
using amx::Lab;

int lab_check_batch(int batch, long long voxels) { return amx::check_rows(batch, voxels, "batch", "ensemble"); }
int lab_check_dims(int batch, int d, int h, int w) { return amx::check_rows_dims(batch, d, h, w, "batch", "ensemble"); }
size_t lab_max_bytes(int batch, long long voxels) { return (size_t)batch * Lab::chunks(batch, voxels) * sizeof(int); }

int lab_check_flags(const amx_labels_ensemble* t, int batch) {
  for (int i = 0; i < batch; ++i) {
    if (t[i].flags & ~(AMX_LABELS_MASK | AMX_LABELS_ENVELOPE)) return fail(AMX_ERR_INVALID, "ensemble %d: unknown flags %d", i, t[i].flags);
    if ((t[i].flags & AMX_LABELS_ENVELOPE) && !(t[i].flags & AMX_LABELS_MASK))
      return fail(AMX_ERR_INVALID, "ensemble %d: an envelope needs the foreground mask", i);
  }
  return AMX_OK;
}

// tiles of the two stencil kernels: x on grid.x, (z, y) tiles on grid.y, the ensemble on grid.z
int lab_stencil_grid(int batch, int d, int h, int w, int tx, int ty, int tz, dim3& grid, int& tiles_y) {
  tiles_y = amx::cdiv(h, ty);
  const long long gy = (long long)tiles_y * amx::cdiv(d, tz);
  if (gy > 65535 || batch > 65535) return fail(AMX_ERR_SHAPE, "%d x %d x %d with batch %d has too many tiles for one launch", d, h, w, batch);
  grid = dim3(amx::cdiv(w, tx), (unsigned)gy, batch);
  return AMX_OK;
}
}  // namespace

extern "C" {

size_t amx_labels_template_bytes(void) { return sizeof(amx_labels_template); }
size_t amx_labels_ensemble_bytes(void) { return sizeof(amx_labels_ensemble); }

size_t amx_labels_scratch_bytes(int batch, long long voxels) {
  if (!amx::rows_ok(batch, voxels)) return 0;
  return lab_max_bytes(batch, voxels);
}

int amx_labels_compose(const unsigned char* d_templates, size_t template_bytes, const amx_labels_template* h_templates,
                       const amx_labels_template* d_templates_table, int ntemplates, const amx_labels_ensemble* h_table,
                       const amx_labels_ensemble* d_table, unsigned char* d_out, int batch, int d, int h, int w, void* stream) {
  if (int rc = lab_check_dims(batch, d, h, w)) return rc;
  if (int rc = amx::check_tables(h_table, d_table)) return rc;
  if (int rc = amx::check_tables(h_templates, d_templates_table)) return rc;
  if (!d_templates || !d_out) return fail(AMX_ERR_INVALID, "null templates or output");
  if (ntemplates < 1) return fail(AMX_ERR_INVALID, "ntemplates must be positive (got %d)", ntemplates);
  const int size[3] = {d, h, w};
  for (int i = 0; i < batch; ++i) {
    const amx_labels_ensemble& e = h_table[i];
    if (e.count < 1 || e.count > AMX_LABELS_MAX_TEMPLATES)
      return fail(AMX_ERR_INVALID, "ensemble %d: 1 <= templates <= %d (got %d)", i, AMX_LABELS_MAX_TEMPLATES, e.count);
    if (e.first < 0 || (long long)e.first + e.count > ntemplates)
      return fail(AMX_ERR_INVALID, "ensemble %d: templates %d .. %d are outside the table of %d", i, e.first, e.first + e.count - 1, ntemplates);
  }
  for (int k = 0; k < ntemplates; ++k) {
    const amx_labels_template& t = h_templates[k];
    long long vox = 1;
    for (int a = 0; a < 3; ++a) {
      if (t.crop[a] < 1 || t.before[a] < 0 || t.padded[a] < size[a] || t.padded[a] > (1 << 20) || (long long)t.before[a] + t.crop[a] > t.padded[a])
        return fail(AMX_ERR_INVALID, "template %d axis %d: crop %d, pad-before %d, padded %d for a size of %d", k, a, t.crop[a], t.before[a],
                    t.padded[a], size[a]);
      vox *= t.crop[a];
      // the source coordinate must stay far inside what a 64-bit integer index holds
      double reach = fabs(t.affine[4 * a + 3]);
      for (int c = 0; c < 3; ++c) reach += fabs(t.affine[4 * a + c]) * size[c];
      if (!(reach < 1e9)) return fail(AMX_ERR_INVALID, "template %d axis %d: the affine map is not finite or reaches past 1e9 voxels", k, a);
    }
    if (t.offset < 0 || (unsigned long long)t.offset + (unsigned long long)vox > template_bytes)
      return fail(AMX_ERR_INVALID, "template %d: bytes %lld .. %lld are outside the buffer of %zu", k, (long long)t.offset, (long long)t.offset + vox,
                  template_bytes);
  }
  const amx::StreamDims g = amx::StreamDims::make(d, h, w);
  const dim3 grid(Lab::chunks(batch, g.V), batch);
  if (g.V % 4 == 0 && amx::aligned4(d_out))
    amx::lab_compose_kernel<true><<<grid, Lab::kThreads, 0, (hipStream_t)stream>>>(g, d_templates, d_templates_table, d_table, d_out);
  else
    amx::lab_compose_kernel<false><<<grid, Lab::kThreads, 0, (hipStream_t)stream>>>(g, d_templates, d_templates_table, d_table, d_out);
  AMX_HIP(hipGetLastError());
  return AMX_OK;
}

int amx_labels_median3(const unsigned char* d_in, unsigned char* d_out, int batch, int d, int h, int w, int require,
                       const amx_labels_ensemble* h_table, const amx_labels_ensemble* d_table, void* stream) {
  if (int rc = lab_check_dims(batch, d, h, w)) return rc;
  if (int rc = amx::check_tables(h_table, d_table)) return rc;
  if (!d_in || !d_out) return fail(AMX_ERR_INVALID, "null input or output");
  if (require & ~(AMX_LABELS_MASK | AMX_LABELS_ENVELOPE)) return fail(AMX_ERR_INVALID, "require: AMX_LABELS_* bits (got %d)", require);
  const size_t bytes = (size_t)batch * d * h * w;
  if (amx::overlap(d_in, bytes, d_out, bytes)) return fail(AMX_ERR_INVALID, "d_in and d_out must not overlap");
  dim3 grid;
  int tiles_y;
  if (int rc = lab_stencil_grid(batch, d, h, w, amx::kMedX, amx::kMedY, amx::kMedZ, grid, tiles_y)) return rc;
  amx::lab_median_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(d, h, w, tiles_y, require, d_in, d_out, d_table);
  AMX_HIP(hipGetLastError());
  return AMX_OK;
}

int amx_labels_sphere_mask(const float* const* d_grids, unsigned char* d_mask, int batch, int size, const amx_labels_ensemble* h_table,
                           const amx_labels_ensemble* d_table, void* stream) {
  if (size < 16 || size > 256 || size % 16) return fail(AMX_ERR_SHAPE, "cubes with size %% 16 == 0, 16 <= size <= 256 (got %d)", size);
  if (int rc = lab_check_dims(batch, size, size, size)) return rc;
  if (int rc = amx::check_tables(h_table, d_table)) return rc;
  if (!d_grids || !d_mask) return fail(AMX_ERR_INVALID, "null grids or mask");
  if (int rc = lab_check_flags(h_table, batch)) return rc;
  for (int i = 0; i < batch; ++i) {
    const amx_labels_ensemble& e = h_table[i];
    if (!(e.flags & AMX_LABELS_MASK)) continue;
    if (e.radius < 0 || e.radius > 4096) return fail(AMX_ERR_INVALID, "ensemble %d: 0 <= radius <= 4096 (got %d)", i, e.radius);
    for (int a = 0; a < 3; ++a)
      if (e.shift[a] < -4096 || e.shift[a] > 4096) return fail(AMX_ERR_INVALID, "ensemble %d: |shift| <= 4096 (got %d)", i, e.shift[a]);
  }
  amx::LabSphere a;
  a.size = size;
  for (int s = 0; s < 3; ++s) {
    if (!d_grids[s]) return fail(AMX_ERR_INVALID, "null coarse grid %d", s);
    if (!amx::aligned4(d_grids[s])) return fail(AMX_ERR_INVALID, "coarse grid %d is not 4-byte aligned", s);
    a.grid[s] = d_grids[s];
    a.rs[s] = (float)(1.0 / (double)((size / 16) << s));
  }
  const amx::StreamDims g = amx::StreamDims::make(size, size, size);
  const dim3 grid(Lab::chunks(batch, g.V), batch);
  if (amx::aligned4(d_mask)) amx::lab_sphere_kernel<true><<<grid, Lab::kThreads, 0, (hipStream_t)stream>>>(a, g, d_mask, d_table);
  else amx::lab_sphere_kernel<false><<<grid, Lab::kThreads, 0, (hipStream_t)stream>>>(a, g, d_mask, d_table);
  AMX_HIP(hipGetLastError());
  return AMX_OK;
}

int amx_labels_apply_mask(unsigned char* d_labels, const unsigned char* d_mask, int* d_max, int batch, long long voxels,
                          const amx_labels_ensemble* h_table, const amx_labels_ensemble* d_table, void* d_scratch, size_t scratch_bytes,
                          void* stream) {
  if (int rc = lab_check_batch(batch, voxels)) return rc;
  if (int rc = amx::check_tables(h_table, d_table)) return rc;
  if (!d_labels || !d_max || !d_scratch) return fail(AMX_ERR_INVALID, "null labels, maximum or scratch");
  if (int rc = lab_check_flags(h_table, batch)) return rc;
  bool any = false;
  for (int i = 0; i < batch; ++i) any |= (h_table[i].flags & AMX_LABELS_MASK) != 0;
  if (any && !d_mask) return fail(AMX_ERR_INVALID, "an ensemble has its mask switched on but d_mask is null");
  if (!amx::aligned4(d_scratch) || !amx::aligned4(d_max)) return fail(AMX_ERR_INVALID, "d_scratch and d_max must be 4-byte aligned");
  if (int rc = amx::need_scratch(lab_max_bytes(batch, voxels), scratch_bytes)) return rc;
  const int nchunk = Lab::chunks(batch, voxels), nt = (int)Lab::tiles(voxels);
  const dim3 grid(nchunk, batch);
  const hipStream_t st = (hipStream_t)stream;
  if (voxels % 4 == 0 && amx::aligned4(d_labels) && amx::aligned4(d_mask))
    amx::lab_apply_kernel<true><<<grid, Lab::kThreads, 0, st>>>(d_labels, d_mask, voxels, nt, d_table, (int*)d_scratch);
  else
    amx::lab_apply_kernel<false><<<grid, Lab::kThreads, 0, st>>>(d_labels, d_mask, voxels, nt, d_table, (int*)d_scratch);
  AMX_HIP(hipGetLastError());
  amx::lab_max_finalize_kernel<<<batch, Lab::kThreads, 0, st>>>((const int*)d_scratch, nchunk, d_max);
  AMX_HIP(hipGetLastError());
  return AMX_OK;
}

int amx_labels_envelope(unsigned char* d_labels, const unsigned char* d_mask, const int* d_max, int batch, int d, int h, int w,
                        const amx_labels_ensemble* h_table, const amx_labels_ensemble* d_table, void* stream) {
  if (int rc = lab_check_dims(batch, d, h, w)) return rc;
  if (d < 2 * amx::kEnvR + 1 || h < 2 * amx::kEnvR + 1 || w < 2 * amx::kEnvR + 1)
    return fail(AMX_ERR_SHAPE, "every axis must be at least %d, so that one reflection suffices (got %d x %d x %d)", 2 * amx::kEnvR + 1, d, h, w);
  if (int rc = amx::check_tables(h_table, d_table)) return rc;
  if (!d_labels || !d_mask || !d_max) return fail(AMX_ERR_INVALID, "null labels, mask or maximum");
  const size_t bytes = (size_t)batch * d * h * w;
  if (amx::overlap(d_labels, bytes, d_mask, bytes)) return fail(AMX_ERR_INVALID, "d_labels and d_mask must not overlap");
  if (int rc = lab_check_flags(h_table, batch)) return rc;
  for (int i = 0; i < batch; ++i)
    if ((h_table[i].flags & AMX_LABELS_ENVELOPE) && (h_table[i].ball < 2 || h_table[i].ball > amx::kEnvR))
      return fail(AMX_ERR_INVALID, "ensemble %d: the ball's radius is 2, 3 or 4 (got %d)", i, h_table[i].ball);
  dim3 grid;
  int tiles_y;
  if (int rc = lab_stencil_grid(batch, d, h, w, amx::kEnvX, amx::kEnvY, amx::kEnvZ, grid, tiles_y)) return rc;
  amx::lab_envelope_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(d, h, w, tiles_y, d_labels, d_mask, d_max, d_table);
  AMX_HIP(hipGetLastError());
  return AMX_OK;
}

int amx_labels_merge_masks(const unsigned char* d_masks, int n, long long voxels, long long stride, const int* h_group,
                           unsigned char* d_merged, unsigned long long* d_sums, int* d_overflow, int accumulate, void* stream) {
  if (n < 1 || n > AMX_LABELS_MAX_MERGE) return fail(AMX_ERR_SHAPE, "1 <= n <= %d mask files per call (got %d)", AMX_LABELS_MAX_MERGE, n);
  if (!amx::row_voxels_ok(voxels)) return fail(AMX_ERR_SHAPE, "1 <= voxels < 2^31 per mask (got %lld)", voxels);
  if (stride < voxels || stride % 16) return fail(AMX_ERR_SHAPE, "stride must be a multiple of 16 and at least voxels (got %lld for %lld)", stride, voxels);
  if (!d_masks || !h_group || !d_merged || !d_sums || !d_overflow) return fail(AMX_ERR_INVALID, "null masks, groups, merged rows, sums or overflow flags");
  if (!amx::aligned16(d_masks) || !amx::aligned16(d_merged)) return fail(AMX_ERR_INVALID, "d_masks and d_merged must be 16-byte aligned");
  if (((uintptr_t)d_sums & 7) || !amx::aligned4(d_overflow)) return fail(AMX_ERR_INVALID, "d_sums must be 8-byte and d_overflow 4-byte aligned");
  if (amx::overlap(d_masks, (size_t)n * stride, d_merged, (size_t)2 * stride)) return fail(AMX_ERR_INVALID, "d_masks and d_merged must not overlap");
  amx::LabMerge a;
  for (int i = 0; i < n; ++i) {
    if (h_group[i] < 0 || h_group[i] > 2) return fail(AMX_ERR_INVALID, "mask %d: group 0 (neither), 1 (rib) or 2 (vertebra) (got %d)", i, h_group[i]);
    a.group[i] = (unsigned char)h_group[i];
  }
  for (int i = n; i < AMX_LABELS_MAX_MERGE; ++i) a.group[i] = 0;
  const hipStream_t st = (hipStream_t)stream;
  int dev = 0;
  AMX_HIP(hipGetDevice(&dev));
  const int cus = amx::device_cus(dev);
  const long long want = ((voxels >> 4) + 255) / 256, cap = (long long)(cus > 0 ? cus : 256) * 8;
  const int blocks = (int)(want < 1 ? 1 : (want < cap ? want : cap));
  AMX_HIP(hipMemsetAsync(d_sums, 0, (size_t)(n + 2) * sizeof(unsigned long long), st));
  if (!accumulate) AMX_HIP(hipMemsetAsync(d_overflow, 0, 2 * sizeof(int), st));
  amx::lab_merge_kernel<<<blocks, 256, 0, st>>>(a, d_masks, n, voxels, stride, d_merged, d_sums, d_overflow, accumulate);
  AMX_HIP(hipGetLastError());
  return AMX_OK;
}

}  // extern "C"
