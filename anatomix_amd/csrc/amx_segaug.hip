// anatomix_amd -- the augmentation chain of segmentation finetuning (anatomix/segmentation/segmentation_utils.py:159-216, MONAI's
// transforms restated from their documented algorithms) on a whole batch:
//   ScaleIntensity, RandAdjustContrast                         one pointwise kernel behind a per-sample min / max
//   RandSpatialCrop + RandGaussianNoise + RandBiasField        one gather pass, the twelve Legendre values and one exp per voxel
//   RandGaussianSmooth, RandGaussianSharpen                    separable passes, radius <= 4, zero padding
//   RandAffine of image (trilinear, zeros) and label (nearest) one kernel, which also leaves the min / max partials of its output
// fp32 planar [B][1][V], labels uint8.  One launch per stage with the sample on grid.y; what differs per sample (switches
// included) is read from a device table of amx_segaug_sample records, so no stage depends on the host and the launch count
// does not depend on B.  A thread owns four voxels: four consecutive ones behind one 16-byte access where V % 4 == 0 and the bases
// are aligned, otherwise four voxels 256 apart.  Minimum and maximum cross workgroups through a partial slab and a finalize launch.
#include <math.h>
#include <stdio.h>

#include "amx_device.h"
#include "amx_launch.h"
#include "amx_stream.h"

namespace amx {

using Aug = StreamTile<>;                  // a thread owns four voxels of a tile of 1024 (amx_stream.h)
constexpr int kAugMaxRadius = 4;
using AugSample = amx_segaug_sample;

// ---- minimum and maximum --------------------------------------------------------------------------------------------------
// partial pairs of n rows of V floats; CLIP: of max(x, 0) (datagen's ThresholdIntensity folded in, amx_synth.hip)
template <bool VEC, bool CLIP>
__global__ __launch_bounds__(Aug::kThreads) void minmax_kernel(const float* __restrict__ x, long long V, int ntiles, float* __restrict__ part) {
  const float* row = x + (long long)blockIdx.y * V;
  float lo = INFINITY, hi = -INFINITY;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    float v[Aug::kVpt];
    Aug::load4<VEC>(row, t, V, v);
#pragma unroll
    for (int j = 0; j < Aug::kVpt; ++j)
      if (Aug::voxel<VEC>(t, j) < V) {
        const float c = CLIP ? fmaxf(v[j], 0.f) : v[j];
        lo = fminf(lo, c), hi = fmaxf(hi, c);
      }
  }
  block_minmax(lo, hi, minmax_slab(part));
}

// grid (B): minmax[n] = {min, max} over the sample's nchunk partial pairs
__global__ __launch_bounds__(Aug::kThreads) void minmax_finalize_kernel(const float* __restrict__ part, int nchunk, float* __restrict__ minmax) {
  const int n = blockIdx.x;
  float lo = INFINITY, hi = -INFINITY;
  for (int c = threadIdx.x; c < nchunk; c += Aug::kThreads) {
    const float* p = part + ((long long)n * nchunk + c) * 2;
    lo = fminf(lo, p[0]), hi = fmaxf(hi, p[1]);
  }
  block_minmax(lo, hi, minmax + 2 * n);
}

// ---- ScaleIntensity / AdjustContrast ----------------------------------------------------------------------------------------
template <bool VEC, int OP>
__global__ __launch_bounds__(Aug::kThreads) void aug_pointwise_kernel(const float* in, float* out, long long V, int ntiles,
                                                                    const float* __restrict__ minmax, const AugSample* __restrict__ table) {
  const int n = blockIdx.y;
  const AugSample& s = table[n];
  const bool on = s.flags & (OP == AMX_SEGAUG_OP_SCALE ? AMX_SEGAUG_RESCALE : AMX_SEGAUG_CONTRAST);
  const float mn = minmax[2 * n], mx = minmax[2 * n + 1], range = mx - mn, gamma = s.gamma;
  const float* src = in + (long long)n * V;
  float* dst = out + (long long)n * V;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    float v[Aug::kVpt];
    Aug::load4<VEC>(src, t, V, v);
    if (on) {
#pragma unroll
      for (int j = 0; j < Aug::kVpt; ++j) {
        if (OP == AMX_SEGAUG_OP_SCALE) v[j] = mn == mx ? v[j] * 0.f : (v[j] - mn) / range;
        else v[j] = powf((v[j] - mn) / (range + 1e-7f), gamma) * range + mn;
      }
    }
    Aug::store4<VEC>(dst, t, V, v);
  }
}

// ---- crop gather + noise + bias field ----------------------------------------------------------------------------------------
__device__ __forceinline__ void aug_legendre(float x, float (&p)[4]) {
  p[0] = 1.f, p[1] = x, p[2] = 0.5f * (3.f * x * x - 1.f), p[3] = 0.5f * (5.f * x * x * x - 3.f * x);
}

template <bool VEC, int LT>
__global__ __launch_bounds__(Aug::kThreads) void aug_crop_kernel(StreamDims g, const float* __restrict__ noise, float* __restrict__ img,
                                                               unsigned char* __restrict__ lab, const AugSample* __restrict__ table) {
  const int n = blockIdx.y;
  const AugSample& s = table[n];
  const float* vol = s.vol;
  const int H = s.vol_dim[1], W = s.vol_dim[2], cz = s.corner[0], cy = s.corner[1], cx = s.corner[2];
  const bool do_noise = s.flags & AMX_SEGAUG_NOISE, do_bias = s.flags & AMX_SEGAUG_BIAS;
  const float std = s.noise_std;
  float c[20];
#pragma unroll
  for (int i = 0; i < 20; ++i) c[i] = s.bias[i];
  const long long base = (long long)n * g.V;
  for (int t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    float v[Aug::kVpt];
    unsigned char l[Aug::kVpt];
#pragma unroll
    for (int j = 0; j < Aug::kVpt; ++j) {
      const long long o = Aug::voxel<VEC>(t, j);
      v[j] = 0.f, l[j] = 0;
      if (o >= g.V) continue;
      int z, y, x;
      g.split(o, z, y, x);
      const long long src = ((long long)(cz + z) * H + (cy + y)) * W + (cx + x);
      float a = vol[src];
      l[j] = LT == AMX_SEG_LABEL_F32 ? (unsigned char)(int)((const float*)s.lab)[src] : ((const unsigned char*)s.lab)[src];
      if (do_noise) a += std * noise[base + o];
      if (do_bias) {
        float pz[4], py[4], px[4];
        aug_legendre(lin_coord(z, g.d), pz);
        aug_legendre(lin_coord(y, g.h), py);
        aug_legendre(lin_coord(x, g.w), px);
        a *= expf(poly3_sum(c, pz, py, px));
      }
      v[j] = a;
    }
    Aug::store4<VEC>(img + base, t, g.V, v);
    Aug::store4<VEC>(lab + base, t, g.V, l);
  }
}

// ---- separable Gaussian ------------------------------------------------------------------------------------------------------
// one axis of filter `filt` (0 smooth, 1 sharpen sigma1, 2 sharpen sigma2) for the samples with `bit` on, a copy for the others.
// COMBINE (the last pass of the sharpening): out = b + alpha (b - pass).
template <bool VEC, int AXIS, bool COMBINE>
__global__ __launch_bounds__(Aug::kThreads) void aug_gauss_kernel(StreamDims g, const float* __restrict__ in, float* __restrict__ out,
                                                                const float* __restrict__ b, int filt, int bit,
                                                                const AugSample* __restrict__ table) {
  const int n = blockIdx.y;
  const AugSample& s = table[n];
  const bool on = s.flags & bit;
  const int r = min(max(s.radius[filt][AXIS], 0), kAugMaxRadius);      // the entry refuses more where the switch is on
  float tap[2 * kAugMaxRadius + 1];
  load_centred_taps<kAugMaxRadius>(s.taps[filt][AXIS], r, tap);
  const float alpha = s.sharpen_alpha;
  const long long base = (long long)n * g.V;
  const int len = AXIS == 0 ? g.d : (AXIS == 1 ? g.h : g.w);
  const long long stride = AXIS == 0 ? (long long)g.h * g.w : (AXIS == 1 ? g.w : 1);
  const float* src = in + base;
  for (int t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    float v[Aug::kVpt];
    if (!on) {
      Aug::load4<VEC>(src, t, g.V, v);
    } else {
#pragma unroll
      for (int j = 0; j < Aug::kVpt; ++j) {
        const long long o = Aug::voxel<VEC>(t, j);
        v[j] = 0.f;
        if (o >= g.V) continue;
        const int cpos = (int)((o / stride) % len);
        float acc = 0.f;
#pragma unroll
        for (int k = -kAugMaxRadius; k <= kAugMaxRadius; ++k) {
          const int q = cpos + k;
          if (k >= -r && k <= r && q >= 0 && q < len) acc += tap[k + kAugMaxRadius] * src[o + k * stride];
        }
        if (COMBINE) {
          const float bb = b[base + o];
          acc = bb + alpha * (bb - acc);
        }
        v[j] = acc;
      }
    }
    Aug::store4<VEC>(out + base, t, g.V, v);
  }
}

// ---- affine resample of image and label --------------------------------------------------------------------------------------
// g: the output, in: the input
template <bool VEC>
__global__ __launch_bounds__(Aug::kThreads) void aug_affine_kernel(StreamDims g, StreamDims in, const float* __restrict__ img_in,
                                                                 const unsigned char* __restrict__ lab_in, float* __restrict__ img_out,
                                                                 unsigned char* __restrict__ lab_out, const AugSample* __restrict__ table,
                                                                 float* __restrict__ part) {
  const int n = blockIdx.y;
  const AugSample& s = table[n];
  float A[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) A[i] = s.affine[i];
  const float oz = 0.5f * (g.d - 1), oy = 0.5f * (g.h - 1), ox = 0.5f * (g.w - 1);
  const float iz = 0.5f * (in.d - 1), iy = 0.5f * (in.h - 1), ix = 0.5f * (in.w - 1);
  const float* src = img_in + (long long)n * in.V;
  const unsigned char* lsrc = lab_in + (long long)n * in.V;
  const long long base = (long long)n * g.V;
  float lo = INFINITY, hi = -INFINITY;
  for (int t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    float v[Aug::kVpt];
    unsigned char l[Aug::kVpt];
#pragma unroll
    for (int j = 0; j < Aug::kVpt; ++j) {
      const long long o = Aug::voxel<VEC>(t, j);
      v[j] = 0.f, l[j] = 0;
      if (o >= g.V) continue;
      const float px = (float)(int)(o % g.w) - ox, py = (float)(int)((o / g.w) % g.h) - oy, pz = (float)(int)(o / ((long long)g.w * g.h)) - oz;
      const float sz = A[0] * pz + A[1] * py + A[2] * px + iz;
      const float sy = A[3] * pz + A[4] * py + A[5] * px + iy;
      const float sx = A[6] * pz + A[7] * py + A[8] * px + ix;
      // anything at least one voxel outside the input (NaN included) has no corner and no nearest voxel inside
      if (sz > -1.f && sz < (float)in.d && sy > -1.f && sy < (float)in.h && sx > -1.f && sx < (float)in.w) {
        const float fz0 = floorf(sz), fy0 = floorf(sy), fx0 = floorf(sx);
        const int z0 = (int)fz0, y0 = (int)fy0, x0 = (int)fx0;
        const float fz = sz - fz0, fy = sy - fy0, fx = sx - fx0;
        if (fz == 0.f && fy == 0.f && fx == 0.f) {
          v[j] = src[((long long)z0 * in.h + y0) * in.w + x0];      // z0, y0, x0 >= 0 here: an integral index above -1
        } else {
          float acc = 0.f;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const int zz = z0 + (c >> 2), yy = y0 + ((c >> 1) & 1), xx = x0 + (c & 1);
            const float wgt = ((c >> 2) ? fz : 1.f - fz) * (((c >> 1) & 1) ? fy : 1.f - fy) * ((c & 1) ? fx : 1.f - fx);
            if (zz >= 0 && zz < in.d && yy >= 0 && yy < in.h && xx >= 0 && xx < in.w) acc += wgt * src[((long long)zz * in.h + yy) * in.w + xx];
          }
          v[j] = acc;
        }
        const int nz = (int)rintf(sz), ny = (int)rintf(sy), nx = (int)rintf(sx);
        if (nz >= 0 && nz < in.d && ny >= 0 && ny < in.h && nx >= 0 && nx < in.w) l[j] = lsrc[((long long)nz * in.h + ny) * in.w + nx];
      }
      lo = fminf(lo, v[j]), hi = fmaxf(hi, v[j]);
    }
    Aug::store4<VEC>(img_out + base, t, g.V, v);
    Aug::store4<VEC>(lab_out + base, t, g.V, l);
  }
  block_minmax(lo, hi, minmax_slab(part));
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
size_t minmax_bytes(int n, long long V) { return (size_t)n * Aug::chunks(n, V) * 2 * sizeof(float); }

hipError_t launch_minmax_partials(const float* x, int n, long long V, bool clip, void* scratch, hipStream_t st) {
  const dim3 grid(Aug::chunks(n, V), n);
  const int nt = (int)Aug::tiles(V);
  const bool vec = V % 4 == 0 && aligned16(x);
  if (clip) {
    if (vec) minmax_kernel<true, true><<<grid, Aug::kThreads, 0, st>>>(x, V, nt, (float*)scratch);
    else minmax_kernel<false, true><<<grid, Aug::kThreads, 0, st>>>(x, V, nt, (float*)scratch);
  } else {
    if (vec) minmax_kernel<true, false><<<grid, Aug::kThreads, 0, st>>>(x, V, nt, (float*)scratch);
    else minmax_kernel<false, false><<<grid, Aug::kThreads, 0, st>>>(x, V, nt, (float*)scratch);
  }
  return hipGetLastError();
}

static hipError_t launch_minmax_finalize(const void* scratch, int n, long long V, float* minmax, hipStream_t st) {
  minmax_finalize_kernel<<<n, Aug::kThreads, 0, st>>>((const float*)scratch, Aug::chunks(n, V), minmax);
  return hipGetLastError();
}

hipError_t launch_segaug_pointwise(const float* in, float* out, int n, long long V, const float* minmax, int op, const AugSample* table,
                                   hipStream_t st) {
  const dim3 grid(Aug::chunks(n, V), n);
  const bool vec = V % 4 == 0 && aligned16(in) && aligned16(out);
  const int nt = (int)Aug::tiles(V);
  if (op == AMX_SEGAUG_OP_SCALE) {
    if (vec) aug_pointwise_kernel<true, AMX_SEGAUG_OP_SCALE><<<grid, Aug::kThreads, 0, st>>>(in, out, V, nt, minmax, table);
    else aug_pointwise_kernel<false, AMX_SEGAUG_OP_SCALE><<<grid, Aug::kThreads, 0, st>>>(in, out, V, nt, minmax, table);
  } else {
    if (vec) aug_pointwise_kernel<true, AMX_SEGAUG_OP_CONTRAST><<<grid, Aug::kThreads, 0, st>>>(in, out, V, nt, minmax, table);
    else aug_pointwise_kernel<false, AMX_SEGAUG_OP_CONTRAST><<<grid, Aug::kThreads, 0, st>>>(in, out, V, nt, minmax, table);
  }
  return hipGetLastError();
}

hipError_t launch_segaug_crop(int n, int d, int h, int w, const float* noise, int lt, float* img, unsigned char* lab, const AugSample* table,
                              hipStream_t st) {
  const StreamDims g = StreamDims::make(d, h, w);
  const dim3 grid(Aug::chunks(n, g.V), n);
  const bool vec = g.V % 4 == 0 && aligned16(img) && aligned4(lab);
  if (lt == AMX_SEG_LABEL_F32) {
    if (vec) aug_crop_kernel<true, AMX_SEG_LABEL_F32><<<grid, Aug::kThreads, 0, st>>>(g, noise, img, lab, table);
    else aug_crop_kernel<false, AMX_SEG_LABEL_F32><<<grid, Aug::kThreads, 0, st>>>(g, noise, img, lab, table);
  } else {
    if (vec) aug_crop_kernel<true, AMX_SEG_LABEL_U8><<<grid, Aug::kThreads, 0, st>>>(g, noise, img, lab, table);
    else aug_crop_kernel<false, AMX_SEG_LABEL_U8><<<grid, Aug::kThreads, 0, st>>>(g, noise, img, lab, table);
  }
  return hipGetLastError();
}

template <int AXIS, bool COMBINE>
static hipError_t aug_gauss_pass(const StreamDims& g, int n, const float* in, float* out, const float* b, int filt, int bit,
                                 const AugSample* table, hipStream_t st) {
  const dim3 grid(Aug::chunks(n, g.V), n);
  const bool vec = g.V % 4 == 0 && aligned16(in) && aligned16(out);
  if (vec) aug_gauss_kernel<true, AXIS, COMBINE><<<grid, Aug::kThreads, 0, st>>>(g, in, out, b, filt, bit, table);
  else aug_gauss_kernel<false, AXIS, COMBINE><<<grid, Aug::kThreads, 0, st>>>(g, in, out, b, filt, bit, table);
  return hipGetLastError();
}

hipError_t launch_segaug_gaussian(const float* in, float* out, float* tmp, int n, int d, int h, int w, int mode, const AugSample* table,
                                  hipStream_t st) {
  const StreamDims g = StreamDims::make(d, h, w);
  float *t0 = tmp, *t1 = tmp + (long long)n * g.V;
  hipError_t e;
  if (mode == AMX_SEGAUG_GAUSS_SMOOTH) {
    if ((e = aug_gauss_pass<2, false>(g, n, in, t0, nullptr, 0, AMX_SEGAUG_SMOOTH, table, st)) != hipSuccess) return e;
    if ((e = aug_gauss_pass<1, false>(g, n, t0, t1, nullptr, 0, AMX_SEGAUG_SMOOTH, table, st)) != hipSuccess) return e;
    return aug_gauss_pass<0, false>(g, n, t1, out, nullptr, 0, AMX_SEGAUG_SMOOTH, table, st);
  }
  // b = G_1(in) in t0; G_2(b): t0 -> out -> t1, whose last pass reads b and writes out
  if ((e = aug_gauss_pass<2, false>(g, n, in, t0, nullptr, 1, AMX_SEGAUG_SHARPEN, table, st)) != hipSuccess) return e;
  if ((e = aug_gauss_pass<1, false>(g, n, t0, t1, nullptr, 1, AMX_SEGAUG_SHARPEN, table, st)) != hipSuccess) return e;
  if ((e = aug_gauss_pass<0, false>(g, n, t1, t0, nullptr, 1, AMX_SEGAUG_SHARPEN, table, st)) != hipSuccess) return e;
  if ((e = aug_gauss_pass<2, false>(g, n, t0, out, nullptr, 2, AMX_SEGAUG_SHARPEN, table, st)) != hipSuccess) return e;
  if ((e = aug_gauss_pass<1, false>(g, n, out, t1, nullptr, 2, AMX_SEGAUG_SHARPEN, table, st)) != hipSuccess) return e;
  return aug_gauss_pass<0, true>(g, n, t1, out, t0, 2, AMX_SEGAUG_SHARPEN, table, st);
}

hipError_t launch_segaug_affine(const float* img_in, const unsigned char* lab_in, int n, int di, int hi, int wi, float* img_out,
                                unsigned char* lab_out, int d, int h, int w, const AugSample* table, void* scratch, hipStream_t st) {
  const StreamDims g = StreamDims::make(d, h, w);
  const StreamDims in = StreamDims::make(di, hi, wi);
  const dim3 grid(Aug::chunks(n, g.V), n);
  if (g.V % 4 == 0 && aligned16(img_out) && aligned4(lab_out))
    aug_affine_kernel<true><<<grid, Aug::kThreads, 0, st>>>(g, in, img_in, lab_in, img_out, lab_out, table, (float*)scratch);
  else aug_affine_kernel<false><<<grid, Aug::kThreads, 0, st>>>(g, in, img_in, lab_in, img_out, lab_out, table, (float*)scratch);
  return hipGetLastError();
}

}  // namespace amx

namespace {
using amx::fail;
int aug_check_batch(int n, long long voxels) { return amx::check_rows(n, voxels, "n", "sample"); }
int aug_check_dims(int n, int d, int h, int w) { return amx::check_rows_dims(n, d, h, w, "n", "sample"); }
}  // namespace

extern "C" {

size_t amx_segaug_sample_bytes(void) { return sizeof(amx_segaug_sample); }

size_t amx_segaug_scratch_bytes(int n, long long voxels) {
  return amx::rows_ok(n, voxels) ? amx::minmax_bytes(n, voxels) : 0;
}

int amx_segaug_minmax(const float* d_x, int n, long long voxels, float* d_minmax, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (int rc = aug_check_batch(n, voxels)) return rc;
  if (!d_x || !d_minmax || !d_scratch) return fail(AMX_ERR_INVALID, "null input, output or scratch");
  if (int rc = amx::need_scratch(amx::minmax_bytes(n, voxels), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_minmax_partials(d_x, n, voxels, false, d_scratch, (hipStream_t)stream));
  AMX_HIP(amx::launch_minmax_finalize(d_scratch, n, voxels, d_minmax, (hipStream_t)stream));
  return AMX_OK;
}

int amx_segaug_minmax_finalize(const void* d_scratch, size_t scratch_bytes, int n, long long voxels, float* d_minmax, void* stream) {
  if (int rc = aug_check_batch(n, voxels)) return rc;
  if (!d_minmax || !d_scratch) return fail(AMX_ERR_INVALID, "null output or scratch");
  if (int rc = amx::need_scratch(amx::minmax_bytes(n, voxels), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_minmax_finalize(d_scratch, n, voxels, d_minmax, (hipStream_t)stream));
  return AMX_OK;
}

int amx_segaug_pointwise(const float* d_in, float* d_out, int n, long long voxels, const float* d_minmax, int op,
                         const amx_segaug_sample* h_table, const amx_segaug_sample* d_table, void* stream) {
  if (int rc = aug_check_batch(n, voxels)) return rc;
  if (int rc = amx::check_tables(h_table, d_table)) return rc;
  if (!d_in || !d_out || !d_minmax) return fail(AMX_ERR_INVALID, "null input, output or statistics");
  if (op != AMX_SEGAUG_OP_SCALE && op != AMX_SEGAUG_OP_CONTRAST) return fail(AMX_ERR_INVALID, "op: AMX_SEGAUG_OP_SCALE or _CONTRAST (got %d)", op);
  if (op == AMX_SEGAUG_OP_CONTRAST)
    for (int i = 0; i < n; ++i)
      if ((h_table[i].flags & AMX_SEGAUG_CONTRAST) && !(amx::is_finite(h_table[i].gamma) && h_table[i].gamma > 0.f))
        return fail(AMX_ERR_INVALID, "sample %d: gamma must be positive and finite (got %g)", i, (double)h_table[i].gamma);
  AMX_HIP(amx::launch_segaug_pointwise(d_in, d_out, n, voxels, d_minmax, op, d_table, (hipStream_t)stream));
  return AMX_OK;
}

int amx_segaug_crop(int n, int d, int h, int w, const float* d_noise, int label_dtype, float* d_img, unsigned char* d_lab,
                    const amx_segaug_sample* h_table, const amx_segaug_sample* d_table, void* stream) {
  if (int rc = aug_check_dims(n, d, h, w)) return rc;
  if (int rc = amx::check_tables(h_table, d_table)) return rc;
  if (!d_img || !d_lab) return fail(AMX_ERR_INVALID, "null output");
  if (label_dtype != AMX_SEG_LABEL_F32 && label_dtype != AMX_SEG_LABEL_U8)
    return fail(AMX_ERR_INVALID, "label_dtype: AMX_SEG_LABEL_F32 or AMX_SEG_LABEL_U8 (got %d)", label_dtype);
  const int size[3] = {d, h, w};
  for (int i = 0; i < n; ++i) {
    const amx_segaug_sample& s = h_table[i];
    if (!s.vol || !s.lab) return fail(AMX_ERR_INVALID, "sample %d: null volume or label map", i);
    for (int a = 0; a < 3; ++a)
      if (s.vol_dim[a] < 1 || s.corner[a] < 0 || (long long)s.corner[a] + size[a] > s.vol_dim[a])
        return fail(AMX_ERR_SHAPE, "sample %d axis %d: crop [%d, %d + %d) leaves the volume of %d", i, a, s.corner[a], s.corner[a], size[a],
                    s.vol_dim[a]);
    if ((long long)s.vol_dim[0] * s.vol_dim[1] * s.vol_dim[2] >= amx::kMaxRowVoxels) return fail(AMX_ERR_SHAPE, "sample %d: volume of 2^31 voxels or more", i);
    if ((s.flags & AMX_SEGAUG_NOISE) && !d_noise) return fail(AMX_ERR_INVALID, "sample %d has AMX_SEGAUG_NOISE but d_noise is null", i);
    if ((s.flags & AMX_SEGAUG_NOISE) && !amx::is_finite(s.noise_std)) return fail(AMX_ERR_INVALID, "sample %d: noise_std is not finite", i);
    if (s.flags & AMX_SEGAUG_BIAS)
      for (int q = 0; q < 20; ++q)
        if (!amx::is_finite(s.bias[q])) return fail(AMX_ERR_INVALID, "sample %d: bias coefficient %d is not finite", i, q);
  }
  AMX_HIP(amx::launch_segaug_crop(n, d, h, w, d_noise, label_dtype, d_img, d_lab, d_table, (hipStream_t)stream));
  return AMX_OK;
}

int amx_segaug_gaussian(const float* d_in, float* d_out, float* d_tmp, int n, int d, int h, int w, int mode,
                        const amx_segaug_sample* h_table, const amx_segaug_sample* d_table, void* stream) {
  if (int rc = aug_check_dims(n, d, h, w)) return rc;
  if (int rc = amx::check_tables(h_table, d_table)) return rc;
  if (!d_in || !d_out || !d_tmp) return fail(AMX_ERR_INVALID, "null input, output or temporary");
  if (mode != AMX_SEGAUG_GAUSS_SMOOTH && mode != AMX_SEGAUG_GAUSS_SHARPEN)
    return fail(AMX_ERR_INVALID, "mode: AMX_SEGAUG_GAUSS_SMOOTH or _SHARPEN (got %d)", mode);
  const size_t bytes = (size_t)n * d * h * w * sizeof(float);
  if (amx::overlap(d_in, bytes, d_out, bytes) || amx::overlap(d_in, bytes, d_tmp, 2 * bytes) || amx::overlap(d_out, bytes, d_tmp, 2 * bytes))
    return fail(AMX_ERR_INVALID, "d_in, d_out and d_tmp must not overlap");
  const int bit = mode == AMX_SEGAUG_GAUSS_SMOOTH ? AMX_SEGAUG_SMOOTH : AMX_SEGAUG_SHARPEN;
  const int f0 = mode == AMX_SEGAUG_GAUSS_SMOOTH ? 0 : 1, f1 = mode == AMX_SEGAUG_GAUSS_SMOOTH ? 0 : 2;
  for (int i = 0; i < n; ++i) {
    if (!(h_table[i].flags & bit)) continue;
    for (int f = f0; f <= f1; ++f)
      for (int a = 0; a < 3; ++a) {
        const int r = h_table[i].radius[f][a];
        if (r < 0 || r > amx::kAugMaxRadius)
          return fail(AMX_ERR_INVALID, "sample %d filter %d axis %d: radius %d is outside 0 .. %d (sigma <= 1)", i, f, a, r, amx::kAugMaxRadius);
      }
    if (mode == AMX_SEGAUG_GAUSS_SHARPEN && !amx::is_finite(h_table[i].sharpen_alpha))
      return fail(AMX_ERR_INVALID, "sample %d: sharpen_alpha is not finite", i);
  }
  AMX_HIP(amx::launch_segaug_gaussian(d_in, d_out, d_tmp, n, d, h, w, mode, d_table, (hipStream_t)stream));
  return AMX_OK;
}

int amx_segaug_affine(const float* d_img_in, const unsigned char* d_lab_in, int n, int di, int hi, int wi, float* d_img_out,
                      unsigned char* d_lab_out, int d, int h, int w, const amx_segaug_sample* h_table,
                      const amx_segaug_sample* d_table, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (int rc = aug_check_dims(n, d, h, w)) return rc;
  if (int rc = aug_check_dims(n, di, hi, wi)) return rc;
  if (int rc = amx::check_tables(h_table, d_table)) return rc;
  if (!d_img_in || !d_lab_in || !d_img_out || !d_lab_out || !d_scratch) return fail(AMX_ERR_INVALID, "null input, output or scratch");
  const size_t vin = (size_t)n * di * hi * wi, vout = (size_t)n * d * h * w;
  if (amx::overlap(d_img_in, vin * 4, d_img_out, vout * 4) || amx::overlap(d_lab_in, vin, d_lab_out, vout))
    return fail(AMX_ERR_INVALID, "inputs and outputs must not overlap");
  if (int rc = amx::need_scratch(amx::minmax_bytes(n, (long long)d * h * w), scratch_bytes)) return rc;
  for (int i = 0; i < n; ++i)
    for (int q = 0; q < 9; ++q)
      if (!amx::is_finite(h_table[i].affine[q])) return fail(AMX_ERR_INVALID, "sample %d: affine entry %d is not finite", i, q);
  AMX_HIP(amx::launch_segaug_affine(d_img_in, d_lab_in, n, di, hi, wi, d_img_out, d_lab_out, d, h, w, d_table, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

}  // extern "C"
