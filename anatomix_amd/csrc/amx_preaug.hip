// anatomix_amd -- the two-view augmentation of the contrastive pretraining (pretraining/data/h5supcl_dataset.py:122-178, 260-303,
// TorchIO's transforms restated from their documented algorithms) on one pair:
//   RandomFlip + RandomAffine of both views (trilinear, padded with the view's minimum) and the label (nearest)   one gather kernel
//   RandomBlur, sigma <= 2 (radius <= 8), reflect boundaries                                                      two LDS-tiled kernels
//   RandomNoise, RandomBiasField(order 3), RandomGamma                                                            one pointwise kernel
// fp32 [views][D][H][W], labels uint8.  One launch per stage with the view on grid.y; what differs per view (switches included) is
// read from a device table of amx_preaug_view records.  A view whose switch is off is copied through bit for bit.  Nothing crosses
// threads except through the blur's LDS tiles, and nothing is accumulated across workgroups.
#include <math.h>
#include <stdio.h>

#include "amx_device.h"
#include "amx_launch.h"
#include "amx_stream.h"

namespace amx {

using Pre = StreamTile<>;                  // a thread owns four voxels of a tile of 1024 (amx_stream.h)
using PreView = amx_preaug_view;
constexpr int kPreMaxRadius = AMX_PREAUG_MAX_RADIUS, kPreTaps = 2 * kPreMaxRadius + 1;

// ---- flip + affine (and the rigid moves of the motion artefact) ---------------------------------------------------------------
// source index of output voxel o = M (z, y, x, 1); image: trilinear with `pad` for a corner outside, label: nearest (half to even)
// with 0 outside.  The label follows view 0's map and is written by the workgroups of view 0.
template <bool VEC>
__global__ __launch_bounds__(Pre::kThreads) void pre_spatial_kernel(StreamDims g, const float* __restrict__ in, const unsigned char* __restrict__ lab_in,
                                                                  const float* __restrict__ minmax, float* __restrict__ out,
                                                                  unsigned char* __restrict__ lab_out, const PreView* __restrict__ table) {
  const int n = blockIdx.y;
  const PreView& s = table[n];
  const bool on = s.flags & AMX_PREAUG_SPATIAL, with_lab = n == 0 && lab_in != nullptr;
  float M[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) M[i] = s.map[i];
  const float pad = minmax[2 * n];
  const float* src = in + (long long)n * g.V;
  float* dst = out + (long long)n * g.V;
  for (int t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    float v[Pre::kVpt];
    unsigned char l[Pre::kVpt];
#pragma unroll
    for (int j = 0; j < Pre::kVpt; ++j) {
      const long long o = Pre::voxel<VEC>(t, j);
      v[j] = 0.f, l[j] = 0;
      if (o >= g.V) continue;
      if (!on) {
        v[j] = src[o];
        if (with_lab) l[j] = lab_in[o];
        continue;
      }
      const float px = (float)(int)(o % g.w), py = (float)(int)((o / g.w) % g.h), pz = (float)(int)(o / ((long long)g.w * g.h));
      const float sz = M[0] * pz + M[1] * py + M[2] * px + M[3];
      const float sy = M[4] * pz + M[5] * py + M[6] * px + M[7];
      const float sx = M[8] * pz + M[9] * py + M[10] * px + M[11];
      v[j] = pad;
      // anything at least one voxel outside the input (NaN included) has no corner and no nearest voxel inside
      if (sz > -1.f && sz < (float)g.d && sy > -1.f && sy < (float)g.h && sx > -1.f && sx < (float)g.w) {
        const float fz0 = floorf(sz), fy0 = floorf(sy), fx0 = floorf(sx);
        const int z0 = (int)fz0, y0 = (int)fy0, x0 = (int)fx0;
        const float fz = sz - fz0, fy = sy - fy0, fx = sx - fx0;
        if (fz == 0.f && fy == 0.f && fx == 0.f) {
          v[j] = src[((long long)z0 * g.h + y0) * g.w + x0];      // z0, y0, x0 >= 0 here: an integral index above -1
        } else {
          float acc = 0.f;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const int zz = z0 + (c >> 2), yy = y0 + ((c >> 1) & 1), xx = x0 + (c & 1);
            const float wgt = ((c >> 2) ? fz : 1.f - fz) * (((c >> 1) & 1) ? fy : 1.f - fy) * ((c & 1) ? fx : 1.f - fx);
            const bool inside = zz >= 0 && zz < g.d && yy >= 0 && yy < g.h && xx >= 0 && xx < g.w;
            acc += wgt * (inside ? src[((long long)zz * g.h + yy) * g.w + xx] : pad);
          }
          v[j] = acc;
        }
        if (with_lab) {
          const int nz = (int)rintf(sz), ny = (int)rintf(sy), nx = (int)rintf(sx);
          if (nz >= 0 && nz < g.d && ny >= 0 && ny < g.h && nx >= 0 && nx < g.w) l[j] = lab_in[((long long)nz * g.h + ny) * g.w + nx];
        }
      }
    }
    Pre::store4<VEC>(dst, t, g.V, v);
    if (with_lab) Pre::store4<VEC>(lab_out, t, g.V, l);
  }
}

// ---- Gaussian blur ----------------------------------------------------------------------------------------------------------
// scipy's mode='reflect' (d c b a | a b c d | d c b a) for any integer i, so also where the radius exceeds the axis
__device__ __forceinline__ int pre_reflect(int i, int n) {
  int m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}

// W and H in one kernel over a plane tile of kBlurTH x kBlurTW outputs.  The tile and a halo of 8 on every side are staged in LDS
// once, reflected while staging (the reflected row and column of every staged position are computed once per workgroup); the W pass
// reads the stage and writes the rows the H pass needs; the H pass reads those.  A lane owns a column, a wave a row of 64: every
// LDS access is a 4-byte one at consecutive addresses across the wave (conflict-free; 28 KB of LDS leave five workgroups = 20 waves
// per CU for these narrow reads).
constexpr int kBlurTH = 32, kBlurTW = 64, kBlurSH = kBlurTH + 2 * kPreMaxRadius, kBlurSW = kBlurTW + 2 * kPreMaxRadius;
static_assert(kBlurTW == 64 && Pre::kThreads % kBlurTW == 0, "a wave covers one row of the tile");

struct PreBlurGrid {
  int tiles_x, tiles_y;
};

__global__ __launch_bounds__(Pre::kThreads) void pre_blur_wh_kernel(StreamDims g, PreBlurGrid bg, const float* __restrict__ in, float* __restrict__ out,
                                                                  const PreView* __restrict__ table) {
  __shared__ float stage[kBlurSH][kBlurSW];
  __shared__ float mid[kBlurSH][kBlurTW];
  __shared__ int rowsrc[kBlurSH], colsrc[kBlurSW];
  const int n = blockIdx.y;
  const PreView& s = table[n];
  const bool on = s.flags & AMX_PREAUG_BLUR;
  const int rh = on ? min(max(s.radius[1], 0), kPreMaxRadius) : 0, rw = on ? min(max(s.radius[2], 0), kPreMaxRadius) : 0;
  const int tx = blockIdx.x % bg.tiles_x, ty = (blockIdx.x / bg.tiles_x) % bg.tiles_y, z = blockIdx.x / (bg.tiles_x * bg.tiles_y);
  const int x0 = tx * kBlurTW, y0 = ty * kBlurTH;
  const long long plane = (long long)n * g.V + (long long)z * g.h * g.w;
  const float* src = in + plane;
  float* dst = out + plane;
  const int lx = threadIdx.x % kBlurTW, ly0 = threadIdx.x / kBlurTW;
  constexpr int kRowsPerPass = Pre::kThreads / kBlurTW;
  if (rh == 0 && rw == 0) {                                           // copied through
    for (int y = ly0; y < kBlurTH; y += kRowsPerPass)
      if (y0 + y < g.h && x0 + lx < g.w) dst[(long long)(y0 + y) * g.w + x0 + lx] = src[(long long)(y0 + y) * g.w + x0 + lx];
    return;
  }
  if (threadIdx.x < kBlurSH) rowsrc[threadIdx.x] = pre_reflect(y0 - kPreMaxRadius + (int)threadIdx.x, g.h);
  else if (threadIdx.x >= 64 && threadIdx.x < 64 + kBlurSW) colsrc[threadIdx.x - 64] = pre_reflect(x0 - kPreMaxRadius + (int)threadIdx.x - 64, g.w);
  __syncthreads();
  // rows the H pass reads: [lo, hi) of the stage
  const int lo = kPreMaxRadius - rh, hi = kPreMaxRadius + kBlurTH + rh;
  for (int i = threadIdx.x; i < (hi - lo) * kBlurSW; i += Pre::kThreads) {
    const int row = lo + i / kBlurSW, col = i % kBlurSW;
    stage[row][col] = src[(long long)rowsrc[row] * g.w + colsrc[col]];
  }
  __syncthreads();
  float tap[kPreTaps];
  load_centred_taps<kPreMaxRadius>(s.taps[2], rw, tap);
  for (int row = lo + ly0; row < hi; row += kRowsPerPass) {
    float acc = stage[row][lx + kPreMaxRadius];
    if (rw > 0) {
      acc = 0.f;
#pragma unroll
      for (int k = -kPreMaxRadius; k <= kPreMaxRadius; ++k)
        if (k >= -rw && k <= rw) acc += tap[k + kPreMaxRadius] * stage[row][lx + kPreMaxRadius + k];
    }
    mid[row][lx] = acc;
  }
  __syncthreads();
  load_centred_taps<kPreMaxRadius>(s.taps[1], rh, tap);
  for (int y = ly0; y < kBlurTH; y += kRowsPerPass) {
    float acc = mid[y + kPreMaxRadius][lx];
    if (rh > 0) {
      acc = 0.f;
#pragma unroll
      for (int k = -kPreMaxRadius; k <= kPreMaxRadius; ++k)
        if (k >= -rh && k <= rh) acc += tap[k + kPreMaxRadius] * mid[y + kPreMaxRadius + k][lx];
    }
    if (y0 + y < g.h && x0 + lx < g.w) dst[(long long)(y0 + y) * g.w + x0 + lx] = acc;
  }
}

// D: a workgroup owns 1024 columns of the flattened H x W plane (four per thread, in either access form) and marches along z
// through kBlurZChunk output planes.  The last 2 r + 1 input planes of its columns sit in an LDS ring, so a plane is fetched once
// per chunk (plus 2 r halo planes per chunk) and every tap is an LDS read: one 16-byte read per tap and four voxels in the 16-byte
// form.  A thread reads back only what it wrote itself, so the march needs no barrier.  The next plane is in flight while the
// current one is summed.
constexpr int kBlurZChunk = 32;

template <bool VEC>
__global__ __launch_bounds__(Pre::kThreads) void pre_blur_d_kernel(StreamDims g, int plane_tiles, const float* __restrict__ in, float* __restrict__ out,
                                                                 const PreView* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) float ring[kPreTaps][Pre::kTile];
  const int n = blockIdx.y;
  const PreView& s = table[n];
  const bool on = s.flags & AMX_PREAUG_BLUR;
  const int r = on ? min(max(s.radius[0], 0), kPreMaxRadius) : 0;
  const int t = blockIdx.x % plane_tiles, z0 = (blockIdx.x / plane_tiles) * kBlurZChunk, z1 = min(z0 + kBlurZChunk, g.d);
  const long long HW = (long long)g.h * g.w;
  const float* src = in + (long long)n * g.V;
  float* dst = out + (long long)n * g.V;
  float v[Pre::kVpt];
  if (r == 0) {                                                       // copied through
    for (int z = z0; z < z1; ++z) {
      Pre::load4<VEC>(src + z * HW, t, HW, v);
      Pre::store4<VEC>(dst + z * HW, t, HW, v);
    }
    return;
  }
  float tap[kPreTaps];
#pragma unroll
  for (int j = 0; j < kPreTaps; ++j) tap[j] = j <= 2 * r ? s.taps[0][j] : 0.f;      // tap[j]: offset j - r
  // this thread's four voxels of a plane in a ring slot: one 16-byte access, or four 4-byte ones 256 apart
  auto put = [&](int slot, const float (&x)[Pre::kVpt]) {
    if (VEC) *(f32x4*)&ring[slot][threadIdx.x * Pre::kVpt] = f32x4{x[0], x[1], x[2], x[3]};
    else
#pragma unroll
      for (int j = 0; j < Pre::kVpt; ++j) ring[slot][j * Pre::kThreads + threadIdx.x] = x[j];
  };
  auto get = [&](int slot, float (&x)[Pre::kVpt]) {
    if (VEC) {
      const f32x4 q = *(const f32x4*)&ring[slot][threadIdx.x * Pre::kVpt];
#pragma unroll
      for (int j = 0; j < Pre::kVpt; ++j) x[j] = q[j];
    } else {
#pragma unroll
      for (int j = 0; j < Pre::kVpt; ++j) x[j] = ring[slot][j * Pre::kThreads + threadIdx.x];
    }
  };
  const int slots = 2 * r + 1;
  // input plane z0 - r + i lives in slot i % slots
  for (int i = 0; i < 2 * r; ++i) {
    Pre::load4<VEC>(src + pre_reflect(z0 - r + i, g.d) * HW, t, HW, v);
    put(i, v);
  }
  float nxt[Pre::kVpt];
  Pre::load4<VEC>(src + pre_reflect(z0 + r, g.d) * HW, t, HW, nxt);
  int head = 2 * r, base = 0;                                         // head: slot of plane z + r; base: slot of plane z - r
  for (int z = z0; z < z1; ++z) {
    put(head, nxt);
    if (z + 1 < z1) Pre::load4<VEC>(src + pre_reflect(z + 1 + r, g.d) * HW, t, HW, nxt);
    float acc[Pre::kVpt] = {0.f, 0.f, 0.f, 0.f};
    int sl = base;
#pragma unroll
    for (int j = 0; j < kPreTaps; ++j) {
      if (j <= 2 * r) {
        get(sl, v);
#pragma unroll
        for (int q = 0; q < Pre::kVpt; ++q) acc[q] += tap[j] * v[q];
        sl = sl + 1 == slots ? 0 : sl + 1;
      }
    }
    Pre::store4<VEC>(dst + z * HW, t, HW, acc);
    head = head + 1 == slots ? 0 : head + 1;
    base = base + 1 == slots ? 0 : base + 1;
  }
}

// ---- noise + bias field + gamma ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(Pre::kThreads) void pre_intensity_kernel(StreamDims g, const float* in, const float* __restrict__ noise, float* out,
                                                                    const PreView* __restrict__ table) {
  const int n = blockIdx.y;
  const PreView& s = table[n];
  const bool do_noise = s.flags & AMX_PREAUG_NOISE, do_bias = s.flags & AMX_PREAUG_BIAS, do_gamma = s.flags & AMX_PREAUG_GAMMA;
  const float std = s.noise_std, gamma = s.gamma;
  float c[20];
#pragma unroll
  for (int i = 0; i < 20; ++i) c[i] = s.bias[i];
  const long long base = (long long)n * g.V;
  for (int t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    float v[Pre::kVpt], nz[Pre::kVpt] = {0.f, 0.f, 0.f, 0.f};
    Pre::load4<VEC>(in + base, t, g.V, v);
    if (do_noise) Pre::load4<VEC>(noise + base, t, g.V, nz);
#pragma unroll
    for (int j = 0; j < Pre::kVpt; ++j) {
      const long long o = Pre::voxel<VEC>(t, j);
      if (o >= g.V) continue;
      float a = v[j];
      if (do_noise) a += std * nz[j];
      if (do_bias) {
        int iz, iy, ix;
        g.split(o, iz, iy, ix);
        const float x = lin_coord(ix, g.w), y = lin_coord(iy, g.h), z = lin_coord(iz, g.d);
        const float pz[4] = {1.f, z, z * z, z * z * z}, py[4] = {1.f, y, y * y, y * y * y}, px[4] = {1.f, x, x * x, x * x * x};
        a *= expf(poly3_sum(c, pz, py, px));
      }
      if (do_gamma) a = copysignf(powf(fabsf(a), gamma), a);
      v[j] = a;
    }
    Pre::store4<VEC>(out + base, t, g.V, v);
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
static hipError_t launch_preaug_spatial(const float* in, const unsigned char* lab_in, int views, int d, int h, int w, const float* minmax, float* out,
                                        unsigned char* lab_out, const PreView* table, hipStream_t st) {
  const StreamDims g = StreamDims::make(d, h, w);
  const dim3 grid(Pre::chunks(views, g.V), views);
  if (g.V % 4 == 0 && aligned16(out) && (!lab_out || aligned4(lab_out)))
    pre_spatial_kernel<true><<<grid, Pre::kThreads, 0, st>>>(g, in, lab_in, minmax, out, lab_out, table);
  else pre_spatial_kernel<false><<<grid, Pre::kThreads, 0, st>>>(g, in, lab_in, minmax, out, lab_out, table);
  return hipGetLastError();
}

static long long preaug_blur_wh_blocks(int d, int h, int w) { return (long long)cdiv(w, kBlurTW) * cdiv(h, kBlurTH) * d; }
static long long preaug_blur_d_blocks(int d, int h, int w) { return Pre::tiles((long long)h * w) * cdiv(d, kBlurZChunk); }

static hipError_t launch_preaug_blur(const float* in, float* out, float* tmp, int views, int d, int h, int w, const PreView* table, hipStream_t st) {
  const StreamDims g = StreamDims::make(d, h, w);
  PreBlurGrid bg;
  bg.tiles_x = cdiv(w, kBlurTW), bg.tiles_y = cdiv(h, kBlurTH);
  pre_blur_wh_kernel<<<dim3((unsigned)preaug_blur_wh_blocks(d, h, w), views), Pre::kThreads, 0, st>>>(g, bg, in, tmp, table);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long long HW = (long long)h * w;
  const int plane_tiles = (int)Pre::tiles(HW);
  const dim3 grid((unsigned)preaug_blur_d_blocks(d, h, w), views);
  if (HW % 4 == 0 && aligned16(tmp) && aligned16(out)) pre_blur_d_kernel<true><<<grid, Pre::kThreads, 0, st>>>(g, plane_tiles, tmp, out, table);
  else pre_blur_d_kernel<false><<<grid, Pre::kThreads, 0, st>>>(g, plane_tiles, tmp, out, table);
  return hipGetLastError();
}

static hipError_t launch_preaug_intensity(const float* in, const float* noise, float* out, int views, int d, int h, int w, const PreView* table,
                                          hipStream_t st) {
  const StreamDims g = StreamDims::make(d, h, w);
  const dim3 grid(Pre::chunks(views, g.V), views);
  if (g.V % 4 == 0 && aligned16(in) && aligned16(out) && (!noise || aligned16(noise)))
    pre_intensity_kernel<true><<<grid, Pre::kThreads, 0, st>>>(g, in, noise, out, table);
  else pre_intensity_kernel<false><<<grid, Pre::kThreads, 0, st>>>(g, in, noise, out, table);
  return hipGetLastError();
}

}  // namespace amx

namespace {
using amx::fail;
constexpr int kPreMaxAxis = 1 << 29;                // keeps 2 * axis + halo inside an int (the reflection)

int pre_check(int views, int d, int h, int w, const void* h_table, const void* d_table) {
  if (d > kPreMaxAxis || h > kPreMaxAxis || w > kPreMaxAxis) return fail(AMX_ERR_SHAPE, "an axis above 2^29 (got %d x %d x %d)", d, h, w);
  if (int rc = amx::check_rows_dims(views, d, h, w, "views", "view")) return rc;
  return amx::check_tables(h_table, d_table);
}
}  // namespace

extern "C" {

size_t amx_preaug_view_bytes(void) { return sizeof(amx_preaug_view); }

int amx_preaug_spatial(const float* d_in, const unsigned char* d_lab_in, int views, int d, int h, int w, const float* d_minmax, float* d_out,
                       unsigned char* d_lab_out, const amx_preaug_view* h_table, const amx_preaug_view* d_table, void* stream) {
  if (int rc = pre_check(views, d, h, w, h_table, d_table)) return rc;
  if (!d_in || !d_out || !d_minmax) return fail(AMX_ERR_INVALID, "null input, output or statistics");
  if ((d_lab_in == nullptr) != (d_lab_out == nullptr)) return fail(AMX_ERR_INVALID, "d_lab_in and d_lab_out: both or neither");
  const size_t vox = (size_t)d * h * w;
  if (amx::overlap(d_in, views * vox * 4, d_out, views * vox * 4) || (d_lab_in && amx::overlap(d_lab_in, vox, d_lab_out, vox)))
    return fail(AMX_ERR_INVALID, "inputs and outputs must not overlap");
  for (int i = 0; i < views; ++i)
    if (h_table[i].flags & AMX_PREAUG_SPATIAL)
      for (int q = 0; q < 12; ++q)
        if (!amx::is_finite(h_table[i].map[q])) return fail(AMX_ERR_INVALID, "view %d: map entry %d is not finite", i, q);
  AMX_HIP(amx::launch_preaug_spatial(d_in, d_lab_in, views, d, h, w, d_minmax, d_out, d_lab_out, d_table, (hipStream_t)stream));
  return AMX_OK;
}

int amx_preaug_blur(const float* d_in, float* d_out, float* d_tmp, int views, int d, int h, int w, const amx_preaug_view* h_table,
                    const amx_preaug_view* d_table, void* stream) {
  if (int rc = pre_check(views, d, h, w, h_table, d_table)) return rc;
  if (!d_in || !d_out || !d_tmp) return fail(AMX_ERR_INVALID, "null input, output or temporary");
  const size_t bytes = (size_t)views * d * h * w * sizeof(float);
  if (amx::overlap(d_in, bytes, d_out, bytes) || amx::overlap(d_in, bytes, d_tmp, bytes) || amx::overlap(d_out, bytes, d_tmp, bytes))
    return fail(AMX_ERR_INVALID, "d_in, d_out and d_tmp must not overlap");
  if (amx::preaug_blur_wh_blocks(d, h, w) > 0x7fffffffLL || amx::preaug_blur_d_blocks(d, h, w) > 0x7fffffffLL)
    return fail(AMX_ERR_SHAPE, "%d x %d x %d needs more workgroups than a launch has", d, h, w);
  for (int i = 0; i < views; ++i) {
    if (!(h_table[i].flags & AMX_PREAUG_BLUR)) continue;
    for (int a = 0; a < 3; ++a) {
      const int r = h_table[i].radius[a];
      if (r < 0 || r > AMX_PREAUG_MAX_RADIUS)
        return fail(AMX_ERR_INVALID, "view %d axis %d: radius %d is outside 0 .. %d (sigma <= 2)", i, a, r, AMX_PREAUG_MAX_RADIUS);
      for (int k = 0; k <= 2 * r; ++k)
        if (!amx::is_finite(h_table[i].taps[a][k])) return fail(AMX_ERR_INVALID, "view %d axis %d: tap %d is not finite", i, a, k);
    }
  }
  AMX_HIP(amx::launch_preaug_blur(d_in, d_out, d_tmp, views, d, h, w, d_table, (hipStream_t)stream));
  return AMX_OK;
}

int amx_preaug_intensity(const float* d_in, const float* d_noise, float* d_out, int views, int d, int h, int w, const amx_preaug_view* h_table,
                         const amx_preaug_view* d_table, void* stream) {
  if (int rc = pre_check(views, d, h, w, h_table, d_table)) return rc;
  if (!d_in || !d_out) return fail(AMX_ERR_INVALID, "null input or output");
  const size_t bytes = (size_t)views * d * h * w * sizeof(float);
  if (d_in != d_out && amx::overlap(d_in, bytes, d_out, bytes)) return fail(AMX_ERR_INVALID, "d_out is d_in or does not overlap it");
  if (d_noise && amx::overlap(d_noise, bytes, d_out, bytes)) return fail(AMX_ERR_INVALID, "d_noise must not overlap d_out");
  for (int i = 0; i < views; ++i) {
    const amx_preaug_view& s = h_table[i];
    if ((s.flags & AMX_PREAUG_NOISE) && !d_noise) return fail(AMX_ERR_INVALID, "view %d has AMX_PREAUG_NOISE but d_noise is null", i);
    if ((s.flags & AMX_PREAUG_NOISE) && !amx::is_finite(s.noise_std)) return fail(AMX_ERR_INVALID, "view %d: noise_std is not finite", i);
    if (s.flags & AMX_PREAUG_BIAS)
      for (int q = 0; q < 20; ++q)
        if (!amx::is_finite(s.bias[q])) return fail(AMX_ERR_INVALID, "view %d: bias coefficient %d is not finite", i, q);
    if ((s.flags & AMX_PREAUG_GAMMA) && !(amx::is_finite(s.gamma) && s.gamma > 0.f))
      return fail(AMX_ERR_INVALID, "view %d: gamma must be positive and finite (got %g)", i, (double)s.gamma);
  }
  AMX_HIP(amx::launch_preaug_intensity(d_in, d_noise, d_out, views, d, h, w, d_table, (hipStream_t)stream));
  return AMX_OK;
}

}  // extern "C"
