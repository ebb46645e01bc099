// anatomix_amd -- step 2 of the reference's synthetic data generation (synthetic-data-generation/step2_generate_views.py with
// datagen_utils.py:475-646) on a batch of label maps, two views per label map:
//   appearance pass 1   g = max(std[rank] z + mean[rank], 0) from labels and noise, not stored: its min / max per (sample, view)
//   appearance pass 2   view = (g - min) / (max - min) * (1 + f P), P the sum of the trilinearly upsampled coarse grids evaluated
//                       on the fly; writes the view once and leaves the min / max partials of what it wrote
//   k-space spike       mean of log(|k| + 1e-10) (two-level, double), then one plane wave added in place: no inverse FFT
//   low resolution      nearest-exact down and trilinear up as one 8-tap gather; the low-resolution volume is never written
//   tail                max(x, 0) folded into the min / max pass and into the last ScaleIntensity, which can write uint8
// fp32 planar rows [n][V] with n = 2 batch (row = 2 sample + view), labels uint8 [batch][V].  One launch per stage with the row on
// grid.y; what differs per row is read from a device table of amx_synth_view records.  A thread owns four voxels of a tile of
// 1024 (amx_stream.h): one 16-byte access where V % 4 == 0 and the bases are aligned, four voxels 256 apart otherwise.  Minimum and
// maximum leave per-workgroup partials in the one layout of amx_stream.h, which amx_segaug_minmax_finalize reads.  No float atomics: two runs agree bit for bit.
#include <math.h>
#include <stdio.h>

#include "amx_device.h"
#include "amx_launch.h"
#include "amx_stream.h"

namespace amx {

using Syn = StreamTile<>;
using SynView = amx_synth_view;
constexpr int kSynMaxLdsFloats = 12288;      // 48 KiB of collapsed coarse rows per workgroup, the two label tables besides

// mean and std by LABEL (through the rank table) into LDS; rank 0 of a view with a zero background gets (0, 0), so that g is exactly 0
__device__ __forceinline__ void syn_label_tables(const SynView& s, float* __restrict__ lmean, float* __restrict__ lstd) {
  const bool zero_bg = s.flags & AMX_SYNTH_ZERO_BACKGROUND;
  for (int l = threadIdx.x; l < 256; l += Syn::kThreads) {
    const int r = s.rank[l];
    const bool off = zero_bg && r == 0;
    lmean[l] = off ? 0.f : s.mean[r];
    lstd[l] = off ? 0.f : s.std[r];
  }
  __syncthreads();
}

__device__ __forceinline__ float syn_gmm(float z, int label, const float* lmean, const float* lstd) {
  return fmaxf(lstd[label] * z + lmean[label], 0.f);
}

// ---- appearance pass 1 -------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(Syn::kThreads) void syn_gmm_minmax_kernel(const unsigned char* __restrict__ labels, const float* __restrict__ noise,
                                                                     long long V, int ntiles, const SynView* __restrict__ table,
                                                                     float* __restrict__ part) {
  __shared__ float lmean[256], lstd[256];
  const int row = blockIdx.y;
  syn_label_tables(table[row], lmean, lstd);
  const unsigned char* lab = labels + (long long)(row >> 1) * V;
  const float* z = noise + (long long)row * V;
  float lo = INFINITY, hi = -INFINITY;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    float v[Syn::kVpt];
    int l[Syn::kVpt];
    Syn::load4<VEC>(z, t, V, v);
    Syn::load4<VEC>(lab, t, V, l);
#pragma unroll
    for (int j = 0; j < Syn::kVpt; ++j)
      if (Syn::voxel<VEC>(t, j) < V) {
        const float g = syn_gmm(v[j], l[j], lmean, lstd);
        lo = fminf(lo, g), hi = fmaxf(hi, g);
      }
  }
  block_minmax(lo, hi, minmax_slab(part));
}

// ---- appearance pass 2 -------------------------------------------------------------------------------------------------------
struct SynApp : StreamDims {
  explicit SynApp(const StreamDims& g) : StreamDims(g) {}
  int nscales, sumcw, maxrows;
  float rs[AMX_SYNTH_MAX_SCALES];                // 1 / scale
  int cd[AMX_SYNTH_MAX_SCALES], ch[AMX_SYNTH_MAX_SCALES], cw[AMX_SYNTH_MAX_SCALES], off[AMX_SYNTH_MAX_SCALES + 1];
  const float* grid[AMX_SYNTH_MAX_SCALES];       // [n][cd][ch][cw], already multiplied by its std
};

// A tile of 1024 consecutive voxels lies in at most `maxrows` rows (z, y) of the volume.  For those rows the coarse grids are
// interpolated along z and y first, which leaves one coarse row of cw values per scale and volume row in LDS; a voxel then blends
// two of them per scale.  The coarse grids themselves are a few KiB and are read through the caches.
template <bool VEC>
__global__ __launch_bounds__(Syn::kThreads) void syn_appearance_kernel(SynApp a, const unsigned char* __restrict__ labels,
                                                                     const float* __restrict__ noise, const float* __restrict__ gmm_minmax,
                                                                     float* __restrict__ out, const SynView* __restrict__ table,
                                                                     float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float syn_lds[];
  float *lmean = syn_lds, *lstd = syn_lds + 256, *rows = syn_lds + 512;
  const int row = blockIdx.y;
  const SynView& s = table[row];
  syn_label_tables(s, lmean, lstd);
  const float mn = gmm_minmax[2 * row], range = gmm_minmax[2 * row + 1] - mn, mult = s.perl_mult;
  const unsigned char* lab = labels + (long long)(row >> 1) * a.V;
  const float* z = noise + (long long)row * a.V;
  float* dst = out + (long long)row * a.V;
  const int nrows_vol = a.d * a.h;
  float lo = INFINITY, hi = -INFINITY;
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int row0 = (int)(((long long)t * Syn::kTile) / a.w);
    const int nrows = min(a.maxrows, nrows_vol - row0);
    for (int e = threadIdx.x; e < nrows * a.sumcw; e += Syn::kThreads) {
      const int r = e / a.sumcw, q = e - r * a.sumcw;
      int sc = 0;
      while (sc + 1 < a.nscales && q >= a.off[sc + 1]) ++sc;
      const int cx = q - a.off[sc], vz = (row0 + r) / a.h, vy = (row0 + r) - vz * a.h;
      int z0, z1, y0, y1;
      float lz, ly;
      trilinear_src(vz, a.rs[sc], a.cd[sc], z0, z1, lz);
      trilinear_src(vy, a.rs[sc], a.ch[sc], y0, y1, ly);
      const float* g = a.grid[sc] + (long long)row * a.cd[sc] * a.ch[sc] * a.cw[sc] + cx;
      const int sy = a.cw[sc], sz = a.ch[sc] * a.cw[sc];
      const float p0 = (1.f - ly) * g[z0 * sz + y0 * sy] + ly * g[z0 * sz + y1 * sy];
      const float p1 = (1.f - ly) * g[z1 * sz + y0 * sy] + ly * g[z1 * sz + y1 * sy];
      rows[e] = (1.f - lz) * p0 + lz * p1;
    }
    __syncthreads();
    float v[Syn::kVpt];
    int l[Syn::kVpt];
    Syn::load4<VEC>(z, t, a.V, v);
    Syn::load4<VEC>(lab, t, a.V, l);
#pragma unroll
    for (int j = 0; j < Syn::kVpt; ++j) {
      const long long o = Syn::voxel<VEC>(t, j);
      if (o >= a.V) {
        v[j] = 0.f;
        continue;
      }
      const int vr = (int)(o / a.w), x = (int)(o - (long long)vr * a.w);
      const float* cr = rows + (vr - row0) * a.sumcw;
      float P = 0.f;
      for (int sc = 0; sc < a.nscales; ++sc) {
        int x0, x1;
        float lx;
        trilinear_src(x, a.rs[sc], a.cw[sc], x0, x1, lx);
        P += (1.f - lx) * cr[a.off[sc] + x0] + lx * cr[a.off[sc] + x1];
      }
      const float g = syn_gmm(v[j], l[j], lmean, lstd);
      v[j] = (g - mn) / range * (1.f + mult * P);
      lo = fminf(lo, v[j]), hi = fmaxf(hi, v[j]);
    }
    Syn::store4<VEC>(dst, t, a.V, v);
    __syncthreads();      // the rows of this tile are read: the next tile may overwrite them
  }
  block_minmax(lo, hi, minmax_slab(part));
}

// ---- k-space spike ---------------------------------------------------------------------------------------------------------
// sum over a row of k (complex, interleaved) of log(|k| + 1e-10), in double: a thread owns two consecutive values per half tile
// in both access forms, so the order of the sum does not depend on the alignment
template <bool VEC>
__global__ __launch_bounds__(Syn::kThreads) void syn_logk_kernel(const float* __restrict__ k, long long V, int ntiles, double* __restrict__ part) {
  __shared__ double red[Syn::kThreads];
  const float* row = k + 2 * (long long)blockIdx.y * V;
  double acc = 0.0;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long long o = (long long)t * Syn::kTile + j * (Syn::kTile / 2) + threadIdx.x * 2;
      float c[4] = {1.f, 0.f, 1.f, 0.f};
      if (VEC) {
        if (o < V) {
          const f32x4 q = *(const f32x4*)(row + 2 * o);
          c[0] = q[0], c[1] = q[1], c[2] = q[2], c[3] = q[3];
        }
      } else {
        if (o < V) c[0] = row[2 * o], c[1] = row[2 * o + 1];
        if (o + 1 < V) c[2] = row[2 * o + 2], c[3] = row[2 * o + 3];
      }
      if (o < V) acc += (double)logf(sqrtf(c[0] * c[0] + c[1] * c[1]) + 1e-10f);
      if (o + 1 < V) acc += (double)logf(sqrtf(c[2] * c[2] + c[3] * c[3]) + 1e-10f);
    }
  const double sum = block_tree_sum<double, Syn::kThreads>(acc, red);
  if (threadIdx.x == 0) part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// grid (rows): mean[row] over the row's nchunk partial sums, in a fixed order
__global__ __launch_bounds__(Syn::kThreads) void syn_logk_finalize_kernel(const double* __restrict__ part, int nchunk, long long V, float* __restrict__ mean) {
  __shared__ double red[Syn::kThreads];
  double acc = 0.0;
  for (int c = threadIdx.x; c < nchunk; c += Syn::kThreads) acc += part[(long long)blockIdx.x * nchunk + c];
  const double sum = block_tree_sum<double, Syn::kThreads>(acc, red);
  if (threadIdx.x == 0) mean[blockIdx.x] = (float)(sum / (double)V);
}

// x += Re(delta / N exp(2 pi i sum_a f_a r_a / n_a)) for the rows with AMX_SYNTH_SPIKE; the others are not touched
template <bool VEC>
__global__ __launch_bounds__(Syn::kThreads) void syn_spike_kernel(StreamDims g, float* __restrict__ x, const float* __restrict__ k,
                                                                const float* __restrict__ logk_mean, const SynView* __restrict__ table) {
  const int row = blockIdx.y;
  const SynView& s = table[row];
  if (!(s.flags & AMX_SYNTH_SPIKE)) return;
  const int fz = ((s.spike_loc[0] - g.d / 2) % g.d + g.d) % g.d, fy = ((s.spike_loc[1] - g.h / 2) % g.h + g.h) % g.h,
            fx = ((s.spike_loc[2] - g.w / 2) % g.w + g.w) % g.w;
  const float* kk = k + 2 * ((long long)s.spike_slot * g.V + ((long long)fz * g.h + fy) * g.w + fx);
  const float kre = kk[0], kim = kk[1], mag = sqrtf(kre * kre + kim * kim);
  const float k_int = (s.flags & AMX_SYNTH_SPIKE_FIXED) ? s.spike_intensity : s.spike_factor * 2.5f * logk_mean[s.spike_slot];
  const float amp = expf(k_int), pc = mag > 0.f ? kre / mag : 1.f, ps = mag > 0.f ? kim / mag : 0.f;      // angle(0) = 0
  const float inv = 1.f / (float)g.V, dr = (amp * pc - kre) * inv, di = (amp * ps - kim) * inv;
  const float iz = 1.f / (float)g.d, iy = 1.f / (float)g.h, ix = 1.f / (float)g.w;
  float* dst = x + (long long)row * g.V;
  for (int t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    float v[Syn::kVpt];
    Syn::load4<VEC>(dst, t, g.V, v);
#pragma unroll
    for (int j = 0; j < Syn::kVpt; ++j) {
      const long long o = Syn::voxel<VEC>(t, j);
      if (o >= g.V) continue;
      int vz, vy, vx;
      g.split(o, vz, vy, vx);
      // the phase in turns: every term reduced modulo its axis in integers first
      float turns = (float)(int)(((long long)fz * vz) % g.d) * iz + (float)(int)(((long long)fy * vy) % g.h) * iy +
                    (float)(int)(((long long)fx * vx) % g.w) * ix;
      turns -= floorf(turns);
      float sn, cs;
      sincosf(6.28318530717958647692f * turns, &sn, &cs);
      v[j] += dr * cs - di * sn;
    }
    Syn::store4<VEC>(dst, t, g.V, v);
  }
}

// ---- low resolution ----------------------------------------------------------------------------------------------------------
// one axis of output voxel o: the two low-resolution neighbours as their nearest-exact source voxels, and the weight of the second
__device__ __forceinline__ void syn_lowres_axis(int o, int n, int t, int& s0, int& s1, float& l1) {
  const float sc = (float)t / (float)n, back = (float)n / (float)t;
  const float src = fmaxf(sc * ((float)o + 0.5f) - 0.5f, 0.f);
  const int i0 = min((int)src, t - 1), i1 = min(i0 + 1, t - 1);
  l1 = src - (float)i0;
  s0 = min((int)floorf(((float)i0 + 0.5f) * back), n - 1);
  s1 = min((int)floorf(((float)i1 + 0.5f) * back), n - 1);
}

template <bool VEC>
__global__ __launch_bounds__(Syn::kThreads) void syn_lowres_kernel(StreamDims g, const float* __restrict__ in, float* __restrict__ out,
                                                                 const SynView* __restrict__ table) {
  const int row = blockIdx.y;
  const SynView& s = table[row];
  const bool on = s.flags & AMX_SYNTH_LOWRES;
  const int td = s.lowres[0], th = s.lowres[1], tw = s.lowres[2];
  const float* src = in + (long long)row * g.V;
  float* dst = out + (long long)row * g.V;
  for (int t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    float v[Syn::kVpt];
    if (!on) {
      Syn::load4<VEC>(src, t, g.V, v);
    } else {
#pragma unroll
      for (int j = 0; j < Syn::kVpt; ++j) {
        const long long o = Syn::voxel<VEC>(t, j);
        v[j] = 0.f;
        if (o >= g.V) continue;
        int vz, vy, vx;
        g.split(o, vz, vy, vx);
        int z0, z1, y0, y1, x0, x1;
        float lz, ly, lx;
        syn_lowres_axis(vz, g.d, td, z0, z1, lz);
        syn_lowres_axis(vy, g.h, th, y0, y1, ly);
        syn_lowres_axis(vx, g.w, tw, x0, x1, lx);
        const float* p00 = src + ((long long)z0 * g.h + y0) * g.w;
        const float* p01 = src + ((long long)z0 * g.h + y1) * g.w;
        const float* p10 = src + ((long long)z1 * g.h + y0) * g.w;
        const float* p11 = src + ((long long)z1 * g.h + y1) * g.w;
        const float a0 = (1.f - ly) * ((1.f - lx) * p00[x0] + lx * p00[x1]) + ly * ((1.f - lx) * p01[x0] + lx * p01[x1]);
        const float a1 = (1.f - ly) * ((1.f - lx) * p10[x0] + lx * p10[x1]) + ly * ((1.f - lx) * p11[x0] + lx * p11[x1]);
        v[j] = (1.f - lz) * a0 + lz * a1;
      }
    }
    Syn::store4<VEC>(dst, t, g.V, v);
  }
}

// ---- tail: ThresholdIntensity(above, 0) + ScaleIntensity (+ uint8) -------------------------------------------------------------
template <bool VEC, bool U8>
__global__ __launch_bounds__(Syn::kThreads) void syn_finish_kernel(const float* in, void* out, long long V, int ntiles, const float* __restrict__ minmax) {
  const int row = blockIdx.y;
  const float mn = minmax[2 * row], mx = minmax[2 * row + 1], range = mx - mn;
  const float* src = in + (long long)row * V;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    float v[Syn::kVpt];
    Syn::load4<VEC>(src, t, V, v);
#pragma unroll
    for (int j = 0; j < Syn::kVpt; ++j) {
      const float c = fmaxf(v[j], 0.f);
      v[j] = mn == mx ? c * 0.f : (c - mn) / range;
    }
    if (U8) {
      unsigned char q[Syn::kVpt];
#pragma unroll
      for (int j = 0; j < Syn::kVpt; ++j) q[j] = (unsigned char)(int)(255.f * v[j]);      // truncation, as astype(uint8)
      Syn::store4<VEC>((unsigned char*)out + (long long)row * V, t, V, q);
    } else {
      Syn::store4<VEC>((float*)out + (long long)row * V, t, V, v);
    }
  }
}

}  // namespace amx

namespace {
using amx::fail;
using amx::Syn;
size_t syn_logk_bytes(int n, long long V) { return (size_t)n * Syn::chunks(n, V) * sizeof(double); }

int syn_check_rows(int n, long long voxels) { return amx::check_rows(n, voxels, "rows", "row"); }
int syn_check_dims(int n, int d, int h, int w) { return amx::check_rows_dims(n, d, h, w, "rows", "row"); }
int syn_check_batch(int batch) {
  if (batch < 1 || batch > 32767) return fail(AMX_ERR_SHAPE, "1 <= batch <= 32767 (got %d)", batch);
  return AMX_OK;
}

// the appearance model's part of the records of 2 batch rows
int syn_check_gmm(const amx_synth_view* t, int rows) {
  for (int i = 0; i < rows; ++i) {
    const amx_synth_view& s = t[i];
    if (s.nlabels < 1 || s.nlabels > 256) return fail(AMX_ERR_INVALID, "row %d: 1 <= nlabels <= 256 (got %d)", i, s.nlabels);
    if (s.nlabels == 1 && (s.flags & AMX_SYNTH_ZERO_BACKGROUND))
      return fail(AMX_ERR_INVALID, "row %d: a single label with a zero background is a constant volume (min == max)", i);
    for (int l = 0; l < 256; ++l)
      if (s.rank[l] >= s.nlabels) return fail(AMX_ERR_INVALID, "row %d: rank[%d] = %d is not below nlabels = %d", i, l, s.rank[l], s.nlabels);
    for (int r = 0; r < s.nlabels; ++r)
      if (!amx::is_finite(s.mean[r]) || !amx::is_finite(s.std[r])) return fail(AMX_ERR_INVALID, "row %d: mean or std of rank %d is not finite", i, r);
    if (!amx::is_finite(s.perl_mult)) return fail(AMX_ERR_INVALID, "row %d: perl_mult is not finite", i);
  }
  return AMX_OK;
}
}  // namespace

extern "C" {

size_t amx_synth_view_bytes(void) { return sizeof(amx_synth_view); }

size_t amx_synth_scratch_bytes(int rows, long long voxels) {
  if (!amx::rows_ok(rows, voxels)) return 0;
  const size_t a = amx::minmax_bytes(rows, voxels), b = syn_logk_bytes(rows, voxels);
  return a > b ? a : b;
}

int amx_synth_gmm_minmax(const unsigned char* d_labels, const float* d_noise, int batch, long long voxels, const amx_synth_view* h_table,
                         const amx_synth_view* d_table, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (int rc = syn_check_batch(batch)) return rc;
  const int n = 2 * batch;
  if (int rc = syn_check_rows(n, voxels)) return rc;
  if (int rc = amx::check_tables(h_table, d_table)) return rc;
  if (!d_labels || !d_noise || !d_scratch) return fail(AMX_ERR_INVALID, "null labels, noise or scratch");
  if (int rc = amx::need_scratch(amx::minmax_bytes(n, voxels), scratch_bytes)) return rc;
  if (int rc = syn_check_gmm(h_table, n)) return rc;
  const dim3 grid(Syn::chunks(n, voxels), n);
  const int nt = (int)Syn::tiles(voxels);
  if (voxels % 4 == 0 && amx::aligned16(d_noise) && amx::aligned4(d_labels))
    amx::syn_gmm_minmax_kernel<true><<<grid, Syn::kThreads, 0, (hipStream_t)stream>>>(d_labels, d_noise, voxels, nt, d_table, (float*)d_scratch);
  else
    amx::syn_gmm_minmax_kernel<false><<<grid, Syn::kThreads, 0, (hipStream_t)stream>>>(d_labels, d_noise, voxels, nt, d_table, (float*)d_scratch);
  AMX_HIP(hipGetLastError());
  return AMX_OK;
}

int amx_synth_appearance(const unsigned char* d_labels, const float* d_noise, const float* const* d_grids, const int* scales, int nscales,
                         const float* d_gmm_minmax, float* d_out, int batch, int d, int h, int w, const amx_synth_view* h_table,
                         const amx_synth_view* d_table, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (int rc = syn_check_batch(batch)) return rc;
  const int n = 2 * batch;
  if (int rc = syn_check_dims(n, d, h, w)) return rc;
  if (int rc = amx::check_tables(h_table, d_table)) return rc;
  if (!d_labels || !d_noise || !d_gmm_minmax || !d_out || !d_scratch) return fail(AMX_ERR_INVALID, "null labels, noise, statistics, output or scratch");
  if (nscales < 1 || nscales > AMX_SYNTH_MAX_SCALES || !scales || !d_grids)
    return fail(AMX_ERR_INVALID, "1 <= nscales <= %d with their sizes and grids (got %d)", AMX_SYNTH_MAX_SCALES, nscales);
  const long long V = (long long)d * h * w;
  if (int rc = amx::need_scratch(amx::minmax_bytes(n, V), scratch_bytes)) return rc;
  if (int rc = syn_check_gmm(h_table, n)) return rc;
  amx::SynApp a(amx::StreamDims::make(d, h, w));
  a.nscales = nscales, a.off[0] = 0;
  for (int s = 0; s < AMX_SYNTH_MAX_SCALES; ++s) a.rs[s] = 0.f, a.cd[s] = a.ch[s] = a.cw[s] = 1, a.off[s + 1] = 0, a.grid[s] = nullptr;
  for (int s = 0; s < nscales; ++s) {
    const int sc = scales[s];
    if (sc < 1 || d % sc || h % sc || w % sc)
      return fail(AMX_ERR_SHAPE, "scale %d does not divide %d x %d x %d (the envelope of the reference's `out +=`)", sc, d, h, w);
    if (!d_grids[s]) return fail(AMX_ERR_INVALID, "null coarse grid of scale %d", sc);
    a.rs[s] = (float)(1.0 / (double)sc), a.cd[s] = d / sc, a.ch[s] = h / sc, a.cw[s] = w / sc, a.grid[s] = d_grids[s];
    a.off[s + 1] = a.off[s] + a.cw[s];
  }
  a.sumcw = a.off[nscales];
  a.maxrows = (int)((Syn::kTile - 1 + w - 1) / w + 1);
  if ((long long)a.maxrows * a.sumcw > amx::kSynMaxLdsFloats)
    return fail(AMX_ERR_SHAPE, "w = %d with these scales needs %lld floats of LDS per workgroup (at most %d)", w, (long long)a.maxrows * a.sumcw,
                amx::kSynMaxLdsFloats);
  const size_t lds = (size_t)(512 + a.maxrows * a.sumcw) * sizeof(float);
  const dim3 grid(Syn::chunks(n, V), n);
  if (V % 4 == 0 && amx::aligned16(d_noise) && amx::aligned16(d_out) && amx::aligned4(d_labels))
    amx::syn_appearance_kernel<true><<<grid, Syn::kThreads, lds, (hipStream_t)stream>>>(a, d_labels, d_noise, d_gmm_minmax, d_out, d_table, (float*)d_scratch);
  else
    amx::syn_appearance_kernel<false><<<grid, Syn::kThreads, lds, (hipStream_t)stream>>>(a, d_labels, d_noise, d_gmm_minmax, d_out, d_table, (float*)d_scratch);
  AMX_HIP(hipGetLastError());
  return AMX_OK;
}

int amx_synth_logk_mean(const float* d_k, int rows, long long voxels, float* d_mean, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (int rc = syn_check_rows(rows, voxels)) return rc;
  if (!d_k || !d_mean || !d_scratch) return fail(AMX_ERR_INVALID, "null k-space, output or scratch");
  if (!amx::aligned4(d_k) || ((uintptr_t)d_k & 7)) return fail(AMX_ERR_INVALID, "d_k must be 8-byte aligned (complex64)");
  if (((uintptr_t)d_scratch & 7)) return fail(AMX_ERR_INVALID, "d_scratch must be 8-byte aligned");
  if (int rc = amx::need_scratch(syn_logk_bytes(rows, voxels), scratch_bytes)) return rc;
  const int nchunk = Syn::chunks(rows, voxels), nt = (int)Syn::tiles(voxels);
  const dim3 grid(nchunk, rows);
  if (voxels % 2 == 0 && amx::aligned16(d_k)) amx::syn_logk_kernel<true><<<grid, Syn::kThreads, 0, (hipStream_t)stream>>>(d_k, voxels, nt, (double*)d_scratch);
  else amx::syn_logk_kernel<false><<<grid, Syn::kThreads, 0, (hipStream_t)stream>>>(d_k, voxels, nt, (double*)d_scratch);
  AMX_HIP(hipGetLastError());
  amx::syn_logk_finalize_kernel<<<rows, Syn::kThreads, 0, (hipStream_t)stream>>>((const double*)d_scratch, nchunk, voxels, d_mean);
  AMX_HIP(hipGetLastError());
  return AMX_OK;
}

int amx_synth_spike(float* d_x, const float* d_k, int k_rows, const float* d_logk_mean, int n, int d, int h, int w, const amx_synth_view* h_table,
                    const amx_synth_view* d_table, void* stream) {
  if (int rc = syn_check_dims(n, d, h, w)) return rc;
  if (int rc = amx::check_tables(h_table, d_table)) return rc;
  if (!d_x || !d_k) return fail(AMX_ERR_INVALID, "null image or k-space");
  const int size[3] = {d, h, w};
  for (int i = 0; i < n; ++i) {
    const amx_synth_view& s = h_table[i];
    if (!(s.flags & AMX_SYNTH_SPIKE)) continue;
    if (s.spike_slot < 0 || s.spike_slot >= k_rows) return fail(AMX_ERR_INVALID, "row %d: spike_slot %d is outside the %d rows of d_k", i, s.spike_slot, k_rows);
    for (int a = 0; a < 3; ++a)
      if (s.spike_loc[a] < 0 || s.spike_loc[a] >= size[a])
        return fail(AMX_ERR_INVALID, "row %d axis %d: spike location %d is outside 0 .. %d", i, a, s.spike_loc[a], size[a] - 1);
    if (s.flags & AMX_SYNTH_SPIKE_FIXED) {
      if (!amx::is_finite(s.spike_intensity)) return fail(AMX_ERR_INVALID, "row %d: spike_intensity is not finite", i);
    } else {
      if (!d_logk_mean) return fail(AMX_ERR_INVALID, "row %d takes its intensity from the mean of log|k| but d_logk_mean is null", i);
      if (!amx::is_finite(s.spike_factor)) return fail(AMX_ERR_INVALID, "row %d: spike_factor is not finite", i);
    }
  }
  const amx::StreamDims g = amx::StreamDims::make(d, h, w);
  const dim3 grid(Syn::chunks(n, g.V), n);
  if (g.V % 4 == 0 && amx::aligned16(d_x)) amx::syn_spike_kernel<true><<<grid, Syn::kThreads, 0, (hipStream_t)stream>>>(g, d_x, d_k, d_logk_mean, d_table);
  else amx::syn_spike_kernel<false><<<grid, Syn::kThreads, 0, (hipStream_t)stream>>>(g, d_x, d_k, d_logk_mean, d_table);
  AMX_HIP(hipGetLastError());
  return AMX_OK;
}

int amx_synth_lowres(const float* d_in, float* d_out, int n, int d, int h, int w, const amx_synth_view* h_table, const amx_synth_view* d_table,
                     void* stream) {
  if (int rc = syn_check_dims(n, d, h, w)) return rc;
  if (int rc = amx::check_tables(h_table, d_table)) return rc;
  if (!d_in || !d_out) return fail(AMX_ERR_INVALID, "null input or output");
  const size_t bytes = (size_t)n * d * h * w * sizeof(float);
  if (amx::overlap(d_in, bytes, d_out, bytes)) return fail(AMX_ERR_INVALID, "d_in and d_out must not overlap");
  const int size[3] = {d, h, w};
  for (int i = 0; i < n; ++i)
    if (h_table[i].flags & AMX_SYNTH_LOWRES)
      for (int a = 0; a < 3; ++a)
        if (h_table[i].lowres[a] < 1 || h_table[i].lowres[a] > size[a])
          return fail(AMX_ERR_INVALID, "row %d axis %d: low-resolution size %d is outside 1 .. %d", i, a, h_table[i].lowres[a], size[a]);
  const amx::StreamDims g = amx::StreamDims::make(d, h, w);
  const dim3 grid(Syn::chunks(n, g.V), n);
  if (g.V % 4 == 0 && amx::aligned16(d_in) && amx::aligned16(d_out))
    amx::syn_lowres_kernel<true><<<grid, Syn::kThreads, 0, (hipStream_t)stream>>>(g, d_in, d_out, d_table);
  else amx::syn_lowres_kernel<false><<<grid, Syn::kThreads, 0, (hipStream_t)stream>>>(g, d_in, d_out, d_table);
  AMX_HIP(hipGetLastError());
  return AMX_OK;
}

int amx_synth_clip_minmax(const float* d_x, int n, long long voxels, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (int rc = syn_check_rows(n, voxels)) return rc;
  if (!d_x || !d_scratch) return fail(AMX_ERR_INVALID, "null input or scratch");
  if (int rc = amx::need_scratch(amx::minmax_bytes(n, voxels), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_minmax_partials(d_x, n, voxels, true, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

int amx_synth_finish(const float* d_in, void* d_out, int n, long long voxels, const float* d_minmax, int out_u8, void* stream) {
  if (int rc = syn_check_rows(n, voxels)) return rc;
  if (!d_in || !d_out || !d_minmax) return fail(AMX_ERR_INVALID, "null input, output or statistics");
  const dim3 grid(Syn::chunks(n, voxels), n);
  const int nt = (int)Syn::tiles(voxels);
  const hipStream_t st = (hipStream_t)stream;
  if (out_u8) {
    if (voxels % 4 == 0 && amx::aligned16(d_in) && amx::aligned4(d_out)) amx::syn_finish_kernel<true, true><<<grid, Syn::kThreads, 0, st>>>(d_in, d_out, voxels, nt, d_minmax);
    else amx::syn_finish_kernel<false, true><<<grid, Syn::kThreads, 0, st>>>(d_in, d_out, voxels, nt, d_minmax);
  } else {
    if (voxels % 4 == 0 && amx::aligned16(d_in) && amx::aligned16(d_out)) amx::syn_finish_kernel<true, false><<<grid, Syn::kThreads, 0, st>>>(d_in, d_out, voxels, nt, d_minmax);
    else amx::syn_finish_kernel<false, false><<<grid, Syn::kThreads, 0, st>>>(d_in, d_out, voxels, nt, d_minmax);
  }
  AMX_HIP(hipGetLastError());
  return AMX_OK;
}

}  // extern "C"
