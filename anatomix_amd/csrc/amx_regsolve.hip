// anatomix_amd -- the discrete stage of the registration (SURVEY §8 row f), downstream of amx_regfeat.hip:
//   coupled_convex          anatomix/registration/convex_adam_utils.py:494-552
//   inverse_consistency     convex_adam_utils.py:555-603
//   F.interpolate(trilinear, align_corners=False) of the displacement field, with the flip / scale of
//   instance_optimization.py:206-217 folded in
//   run_stage1_registration instance_optimization.py:122-222 as one enqueue
// fp32 throughout, batch 1, planar [C][h][w][d].  Streaming / stencil work, no MFMA.  The arithmetic follows the
// reference's operation order (no fused multiply-add: see the pragma), so that the discrete choices of the solver are the
// reference's wherever its own fp32 arithmetic decides them.
#include <stdio.h>

#include "amx_device.h"
#include "amx_launch.h"

#pragma clang fp contract(off)

namespace amx {

struct CoupledCoef {
  float c[6];
};

template <int V> struct VecF;
template <> struct VecF<1> {
  float v[1];
  static __device__ __forceinline__ VecF load(const float* p) { return VecF{{*p}}; }
};
template <> struct VecF<4> {
  float v[4];
  static __device__ __forceinline__ VecF load(const float* p) {
    const float4 q = *(const float4*)p;
    return VecF{{q.x, q.y, q.z, q.w}};
  }
};

// raw[c][p] = mesh[c][argmin[p]]: the label gather of the given argmin (iteration 0 when the caller brings one)
__global__ __launch_bounds__(256) void mesh_gather_kernel(const long long* __restrict__ idx, long long plane, int k,
                                                          float* __restrict__ raw) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= plane) return;
  int m = (int)idx[o];
  m = m < 0 ? 0 : (m >= k * k * k ? k * k * k - 1 : m);
  const int hw = k / 2;
  raw[o] = (float)(m % k - hw);
  raw[plane + o] = (float)((m / k) % k - hw);
  raw[2 * plane + o] = (float)(m / (k * k) - hw);
}

// One coupled iteration's argmin with the label gather fused: for V consecutive voxels per thread
//   cost(m) = (((ssd(m) + c_0 |mesh_m - s_0|^2) + c_1 |mesh_m - s_1|^2) + ...) + c_{J-1} |mesh_m - s_{J-1}|^2
// accumulated in the reference's order from the J soft fields kept so far (hist [J][3][plane]); ssd is only read.  The
// label loop runs over memory (one coalesced plane row per label); the 3 J soft values per voxel are the only state.
// mesh_m = (m % k, (m / k) % k, m / k^2) - hw, the exact integers of the reference's affine_grid mesh.
template <int J, int V>
__global__ __launch_bounds__(256) void coupled_argmin_kernel(const float* __restrict__ ssd, const float* __restrict__ hist,
                                                             long long plane, int k, CoupledCoef cc, float* __restrict__ raw,
                                                             long long* __restrict__ label) {
  const long long o = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
  if (o >= plane) return;
  float s[J > 0 ? J : 1][3][V];
#pragma unroll
  for (int i = 0; i < J; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const VecF<V> q = VecF<V>::load(hist + (long long)(i * 3 + c) * plane + o);
#pragma unroll
      for (int e = 0; e < V; ++e) s[i][c][e] = q.v[e];
    }
  const int hw = k / 2;
  float best[V], bm[3][V];
  int bi[V];
  int m = 0;
#pragma unroll 1
  for (int a2 = 0; a2 < k; ++a2)
#pragma unroll 1
    for (int a1 = 0; a1 < k; ++a1)
#pragma unroll 1
      for (int a0 = 0; a0 < k; ++a0, ++m) {
        const float m0 = (float)(a0 - hw), m1 = (float)(a1 - hw), m2 = (float)(a2 - hw);
        const VecF<V> q = VecF<V>::load(ssd + (long long)m * plane + o);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          float v = q.v[e];
#pragma unroll
          for (int i = 0; i < J; ++i) {
            const float d0 = m0 - s[i][0][e], d1 = m1 - s[i][1][e], d2 = m2 - s[i][2][e];
            v = v + cc.c[i] * ((d0 * d0 + d1 * d1) + d2 * d2);
          }
          if (m == 0 || v < best[e]) {          // strict: the first minimum wins, as torch.argmin
            best[e] = v;
            bi[e] = m;
            bm[0][e] = m0;
            bm[1][e] = m1;
            bm[2][e] = m2;
          }
        }
      }
#pragma unroll
  for (int e = 0; e < V; ++e) {
#pragma unroll
    for (int c = 0; c < 3; ++c) raw[(long long)c * plane + o + e] = bm[c][e];
    if (label) label[o + e] = bi[e];
  }
}

// One Jacobi sweep of inverse_consistency for both fields (blockIdx.y = field): out = 0.5 * (own - sample(other, id + own)),
// F.grid_sample defaults (trilinear, zeros outside, align_corners=False); channel 0 is the x (last axis) coordinate.  One
// voxel per thread, consecutive lanes along the row, all 24 corner loads issued before the blends.  (A run of four voxels
// per thread with 16-byte stores was measured 2.4x slower, 1.56 against 0.66 ms for 15 sweeps at 128^3: every gather of a
// wave then spans four times as many cache lines, and the gathers are what the sweep is made of.)
__global__ __launch_bounds__(256) void ic_sweep_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       float* __restrict__ ao, float* __restrict__ bo, int H, int W, int D) {
  const long long plane = (long long)H * W * D, row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= plane) return;
  const int x = (int)(row % D), y = (int)((row / D) % W), z = (int)(row / ((long long)D * W));
  const float* own = blockIdx.y ? b : a;
  const float* oth = blockIdx.y ? a : b;
  float* out = blockIdx.y ? bo : ao;
  const float o0 = own[row], o1 = own[plane + row], o2 = own[2 * plane + row];
  const float gx = identity_coord(x, D) + o0, gy = identity_coord(y, W) + o1, gz = identity_coord(z, H) + o2;
  const float ix = ((gx + 1.f) * (float)D - 1.f) / 2.f, iy = ((gy + 1.f) * (float)W - 1.f) / 2.f,
              iz = ((gz + 1.f) * (float)H - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
  // clamp far outside positions (and NaN) before the integer conversion: every corner is then out of bounds -> 0
  const bool sane = fx >= -2.f && fx <= (float)D && fy >= -2.f && fy <= (float)W && fz >= -2.f && fz <= (float)H;
  const int xw = sane ? (int)fx : -2, yn = sane ? (int)fy : -2, zt = sane ? (int)fz : -2;
  const float wx1 = ix - fx, wx0 = (fx + 1.f) - ix, wy1 = iy - fy, wy0 = (fy + 1.f) - iy, wz1 = iz - fz, wz0 = (fz + 1.f) - iz;
  float v[3][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int xx = xw + (j & 1), yy = yn + ((j >> 1) & 1), zz = zt + (j >> 2);
    const bool in = xx >= 0 && xx < D && yy >= 0 && yy < W && zz >= 0 && zz < H;
    const long long p = in ? ((long long)zz * W + yy) * D + xx : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c][j] = in ? oth[(long long)c * plane + p] : 0.f;
  }
  // corner order and weight products of grid_sampler_3d: tnw, tne, tsw, tse, bnw, bne, bsw, bse
  float wgt[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) wgt[j] = ((j & 1) ? wx1 : wx0) * (((j >> 1) & 1) ? wy1 : wy0) * ((j >> 2) ? wz1 : wz0);
  const float ownv[3] = {o0, o1, o2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += v[c][j] * wgt[j];
    out[(long long)c * plane + row] = 0.5f * (ownv[c] - acc);
  }
}

// out[c] = in[flip ? 2 - c : c] / div[c]: the `(disp_soft / scale).flip(1)` in front of the consistency sweeps
struct Scale3 {
  float v[3];
};
__global__ __launch_bounds__(256) void field_normalize_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                              long long plane, Scale3 div) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= plane) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[(long long)c * plane + o] = __fdiv_rn(in[(long long)(2 - c) * plane + o], div.v[2 - c]);
}

constexpr int kResizeMaxC = 16;
struct ResizeScale {
  float v[kResizeMaxC];
};

__device__ __forceinline__ void linear_src(int dst, float ratio, int in, int& i0, int& i1, float& l0, float& l1) {
  float src = ratio * ((float)dst + 0.5f) - 0.5f;      // PyTorch's area_pixel_compute_source_index, align_corners=False
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  i0 = i0 > in - 1 ? in - 1 : i0;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

// F.interpolate(x_src * scale, size=(H, W, D), mode="trilinear", align_corners=False) with x_src[c] = in[flip ? C-1-c : c]
// and scale per OUTPUT channel: one pass, one output voxel per thread (consecutive lanes along the row), each output written
// once.  (Four outputs per thread with 16-byte stores: 0.20 against 0.15 ms at 3 x 128^3 -> 256^3, for the same reason as in
// the sweep; loading the at most four distinct input columns of those four outputs once and selecting: 0.33 ms.)
__global__ __launch_bounds__(256) void resize_trilinear_kernel(const float* __restrict__ in, int C, int h, int w, int d,
                                                               float* __restrict__ out, int H, int W, int D,
                                                               ResizeScale sc, int flip) {
  const long long iplane = (long long)h * w * d, oplane = (long long)H * W * D, o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= oplane) return;
  const int x = (int)(o % D), y = (int)((o / D) % W), z = (int)(o / ((long long)D * W));
  const float rz = (float)h / (float)H, ry = (float)w / (float)W, rx = (float)d / (float)D;
  int z0, z1, y0, y1, xa, xb;
  float lz0, lz1, ly0, ly1, lx0, lx1;
  linear_src(z, rz, h, z0, z1, lz0, lz1);
  linear_src(y, ry, w, y0, y1, ly0, ly1);
  linear_src(x, rx, d, xa, xb, lx0, lx1);
  const long long r00 = ((long long)z0 * w + y0) * d, r01 = ((long long)z0 * w + y1) * d, r10 = ((long long)z1 * w + y0) * d,
                  r11 = ((long long)z1 * w + y1) * d;
#pragma unroll 1
  for (int c = 0; c < C; ++c) {
    const float* src = in + (long long)(flip ? C - 1 - c : c) * iplane;
    const float s = sc.v[c];
    const float v000 = src[r00 + xa] * s, v001 = src[r00 + xb] * s, v010 = src[r01 + xa] * s, v011 = src[r01 + xb] * s;
    const float v100 = src[r10 + xa] * s, v101 = src[r10 + xb] * s, v110 = src[r11 + xa] * s, v111 = src[r11 + xb] * s;
    out[(long long)c * oplane + o] = lz0 * (ly0 * (lx0 * v000 + lx1 * v001) + ly1 * (lx0 * v010 + lx1 * v011)) +
                                     lz1 * (ly0 * (lx0 * v100 + lx1 * v101) + ly1 * (lx0 * v110 + lx1 * v111));
  }
}


static const CoupledCoef kCoef = {{0.003f, 0.01f, 0.03f, 0.1f, 0.3f, 1.f}};

template <int V>
static void launch_coupled_argmin_v(int J, const float* ssd, const float* hist, long long plane, int k, float* raw,
                                    long long* label, hipStream_t st) {
  const int grid = cdiv(plane / V, 256);
  switch (J) {
    case 0: coupled_argmin_kernel<0, V><<<grid, 256, 0, st>>>(ssd, hist, plane, k, kCoef, raw, label); break;
    case 1: coupled_argmin_kernel<1, V><<<grid, 256, 0, st>>>(ssd, hist, plane, k, kCoef, raw, label); break;
    case 2: coupled_argmin_kernel<2, V><<<grid, 256, 0, st>>>(ssd, hist, plane, k, kCoef, raw, label); break;
    case 3: coupled_argmin_kernel<3, V><<<grid, 256, 0, st>>>(ssd, hist, plane, k, kCoef, raw, label); break;
    case 4: coupled_argmin_kernel<4, V><<<grid, 256, 0, st>>>(ssd, hist, plane, k, kCoef, raw, label); break;
    case 5: coupled_argmin_kernel<5, V><<<grid, 256, 0, st>>>(ssd, hist, plane, k, kCoef, raw, label); break;
    default: coupled_argmin_kernel<6, V><<<grid, 256, 0, st>>>(ssd, hist, plane, k, kCoef, raw, label); break;
  }
}

// scratch of one step: the raw (pre-box) label field
size_t coupled_step_scratch_bytes(int h, int w, int d) { return align_up((size_t)3 * h * w * d * sizeof(float), 256); }
// scratch of the whole solve: the raw field + the six soft fields s_0 .. s_5 that later iterations read
size_t coupled_scratch_bytes(int h, int w, int d) { return coupled_step_scratch_bytes(h, w, d) + align_up((size_t)18 * h * w * d * sizeof(float), 256); }

// iteration j (0 .. 6) from the j soft fields in hist: argmin + label gather, then box3 -> s_out.  Two launches.
hipError_t launch_coupled_step(const float* ssd, const float* hist, int j, int h, int w, int d, int disp_hw, float* s_out,
                               long long* label, void* scratch, hipStream_t st) {
  const long long plane = (long long)h * w * d;
  const int k = 2 * disp_hw + 1;
  float* raw = (float*)scratch;
  if (plane % 4 == 0) launch_coupled_argmin_v<4>(j, ssd, hist, plane, k, raw, label, st);
  else launch_coupled_argmin_v<1>(j, ssd, hist, plane, k, raw, label, st);
  return launch_box_filter(raw, s_out, 3, h, w, d, 3, st);
}

hipError_t launch_coupled_convex(const float* ssd, const long long* argmin, int h, int w, int d, int disp_hw, float* out,
                                 void* scratch, hipStream_t st) {
  const long long plane = (long long)h * w * d;
  const int k = 2 * disp_hw + 1;
  float* raw = (float*)scratch;
  float* hist = (float*)((char*)scratch + coupled_step_scratch_bytes(h, w, d));
  hipError_t e;
  if (argmin) {
    mesh_gather_kernel<<<cdiv(plane, 256), 256, 0, st>>>(argmin, plane, k, raw);
    e = launch_box_filter(raw, hist, 3, h, w, d, 3, st);
  } else {
    e = launch_coupled_step(ssd, hist, 0, h, w, d, disp_hw, hist, nullptr, scratch, st);
  }
  for (int j = 1; j <= 6 && e == hipSuccess; ++j)
    e = launch_coupled_step(ssd, hist, j, h, w, d, disp_hw, j < 6 ? hist + (long long)3 * j * plane : out, nullptr, scratch, st);
  return e;
}

size_t ic_scratch_bytes(int h, int w, int d) { return 2 * align_up((size_t)3 * h * w * d * sizeof(float), 256); }

hipError_t launch_inverse_consistency(const float* f1, const float* f2, int h, int w, int d, int iterations, float* o1,
                                      float* o2, void* scratch, hipStream_t st) {
  const size_t fb = (size_t)3 * h * w * d * sizeof(float);
  if (iterations == 0) {
    hipError_t e = hipMemcpyAsync(o1, f1, fb, hipMemcpyDeviceToDevice, st);
    return e != hipSuccess ? e : hipMemcpyAsync(o2, f2, fb, hipMemcpyDeviceToDevice, st);
  }
  float* y1 = (float*)scratch;
  float* y2 = (float*)((char*)scratch + align_up(fb, 256));
  const float *a = f1, *b = f2;
  const dim3 grid(cdiv((long long)h * w * d, 256), 2);
  for (int t = 0; t < iterations; ++t) {
    const bool to_out = ((iterations - 1 - t) & 1) == 0;      // the last sweep lands in the outputs
    float* na = to_out ? o1 : y1;
    float* nb = to_out ? o2 : y2;
    ic_sweep_kernel<<<grid, 256, 0, st>>>(a, b, na, nb, h, w, d);
    a = na;
    b = nb;
  }
  return hipGetLastError();
}

hipError_t launch_resize_trilinear(const float* in, int C, int h, int w, int d, float* out, int H, int W, int D,
                                   const float* scale, int flip, hipStream_t st) {
  ResizeScale sc;
  for (int c = 0; c < kResizeMaxC; ++c) sc.v[c] = (scale && c < C) ? scale[c] : 1.f;
  resize_trilinear_kernel<<<cdiv((long long)H * W * D, 256), 256, 0, st>>>(in, C, h, w, d, out, H, W, D, sc, flip);
  return hipGetLastError();
}

// stage-1 scratch: [ssd][correlate scratch][argmin][coupled scratch][soft fwd][soft bwd][norm fwd][norm bwd][ic fwd][ic bwd][ic scratch]
struct Stage1Layout {
  size_t ssd, corr, amin, coupled, s1, s2, n1, n2, i1, i2, ic, total;
};
static Stage1Layout stage1_layout(int h, int w, int d, int disp_hw, int ic) {
  const size_t k = 2 * disp_hw + 1, plane = (size_t)h * w * d, field = align_up(3 * plane * sizeof(float), 256);
  Stage1Layout L;
  size_t o = 0;
  L.ssd = o, o += align_up(k * k * k * plane * sizeof(float), 256);
  L.corr = o, o += align_up(correlate_scratch_bytes(h, w, d, disp_hw), 256);
  L.amin = o, o += align_up(plane * sizeof(long long), 256);
  L.coupled = o, o += coupled_scratch_bytes(h, w, d);
  L.s1 = o, o += ic ? field : 0;
  L.s2 = o, o += ic ? field : 0;
  L.n1 = o, o += ic ? field : 0;
  L.n2 = o, o += ic ? field : 0;
  L.i1 = o, o += ic ? field : 0;
  L.i2 = o, o += ic ? field : 0;
  L.ic = o, o += ic ? ic_scratch_bytes(h, w, d) : 0;
  L.total = o;
  return L;
}
size_t stage1_scratch_bytes(int h, int w, int d, int disp_hw, int ic) { return stage1_layout(h, w, d, disp_hw, ic).total; }

hipError_t launch_stage1(const float* fix, const float* mov, int n_ch, int h, int w, int d, int disp_hw, int grid_sp, int ic,
                         int H, int W, int D, float* out, void* scratch, hipStream_t st) {
  const Stage1Layout L = stage1_layout(h, w, d, disp_hw, ic);
  char* base = (char*)scratch;
  float* ssd = (float*)(base + L.ssd);
  long long* amin = (long long*)(base + L.amin);
  const long long plane = (long long)h * w * d;
  hipError_t e = launch_correlate(fix, mov, n_ch, h, w, d, disp_hw, ssd, amin, base + L.corr, st);
  if (e != hipSuccess) return e;
  float* s1 = ic ? (float*)(base + L.s1) : out;
  e = launch_coupled_convex(ssd, amin, h, w, d, disp_hw, s1, base + L.coupled, st);
  if (e != hipSuccess || !ic) return e;
  float* s2 = (float*)(base + L.s2);
  e = launch_correlate(mov, fix, n_ch, h, w, d, disp_hw, ssd, amin, base + L.corr, st);
  if (e != hipSuccess) return e;
  e = launch_coupled_convex(ssd, amin, h, w, d, disp_hw, s2, base + L.coupled, st);
  if (e != hipSuccess) return e;
  // scale = (h - 1, w - 1, d - 1) / 2 per channel of disp_soft (instance_optimization.py:181-187)
  const Scale3 sc = {{(float)(h - 1) / 2.f, (float)(w - 1) / 2.f, (float)(d - 1) / 2.f}};
  float *n1 = (float*)(base + L.n1), *n2 = (float*)(base + L.n2), *i1 = (float*)(base + L.i1), *i2 = (float*)(base + L.i2);
  field_normalize_kernel<<<cdiv(plane, 256), 256, 0, st>>>(s1, n1, plane, sc);
  field_normalize_kernel<<<cdiv(plane, 256), 256, 0, st>>>(s2, n2, plane, sc);
  e = launch_inverse_consistency(n1, n2, h, w, d, 15, i1, i2, base + L.ic, st);
  if (e != hipSuccess) return e;
  const float up[3] = {sc.v[0] * (float)grid_sp, sc.v[1] * (float)grid_sp, sc.v[2] * (float)grid_sp};
  return launch_resize_trilinear(i1, 3, h, w, d, out, H, W, D, up, 1, st);
}

}  // namespace amx

namespace {
using amx::fail;

int grid_check(int h, int w, int d, int disp_hw) {
  if (h < 1 || w < 1 || d < 1) return fail(AMX_ERR_SHAPE, "non-positive shape (%d, %d, %d)", h, w, d);
  if (disp_hw < 1 || disp_hw > 3) return fail(AMX_ERR_INVALID, "disp_hw in {1, 2, 3} (got %d)", disp_hw);
  if ((long long)h * w * d * 343 >= (1LL << 40)) return fail(AMX_ERR_SHAPE, "grid too large");
  return AMX_OK;
}
}  // namespace

extern "C" {

size_t amx_coupled_convex_scratch_bytes(int h, int w, int d) {
  return (h < 1 || w < 1 || d < 1) ? 0 : amx::coupled_scratch_bytes(h, w, d);
}

int amx_coupled_convex(const float* d_ssd, const long long* d_argmin, int h, int w, int d, int disp_hw, float* d_disp_soft,
                       void* d_scratch, size_t scratch_bytes, void* stream) {
  if (!d_ssd || !d_disp_soft || !d_scratch) return fail(AMX_ERR_INVALID, "null argument");
  if (int rc = grid_check(h, w, d, disp_hw)) return rc;
  if (int rc = amx::need_scratch(amx::coupled_scratch_bytes(h, w, d), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_coupled_convex(d_ssd, d_argmin, h, w, d, disp_hw, d_disp_soft, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

size_t amx_coupled_convex_step_scratch_bytes(int h, int w, int d) {
  return (h < 1 || w < 1 || d < 1) ? 0 : amx::coupled_step_scratch_bytes(h, w, d);
}

int amx_coupled_convex_step(const float* d_ssd, const float* d_soft_hist, int j, int h, int w, int d, int disp_hw,
                            float* d_soft_out, long long* d_label, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (!d_ssd || !d_soft_out || !d_scratch || (j > 0 && !d_soft_hist)) return fail(AMX_ERR_INVALID, "null argument");
  if (j < 0 || j > 6) return fail(AMX_ERR_INVALID, "iteration in [0, 6] (got %d)", j);
  if (int rc = grid_check(h, w, d, disp_hw)) return rc;
  if (int rc = amx::need_scratch(amx::coupled_step_scratch_bytes(h, w, d), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_coupled_step(d_ssd, d_soft_hist, j, h, w, d, disp_hw, d_soft_out, d_label, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

size_t amx_inverse_consistency_scratch_bytes(int h, int w, int d) {
  return (h < 1 || w < 1 || d < 1) ? 0 : amx::ic_scratch_bytes(h, w, d);
}

int amx_inverse_consistency(const float* d_field1, const float* d_field2, int h, int w, int d, int iterations, float* d_out1,
                            float* d_out2, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (!d_field1 || !d_field2 || !d_out1 || !d_out2 || !d_scratch) return fail(AMX_ERR_INVALID, "null argument");
  if (d_out1 == d_field1 || d_out1 == d_field2 || d_out2 == d_field1 || d_out2 == d_field2 || d_out1 == d_out2)
    return fail(AMX_ERR_INVALID, "outputs must be distinct from the inputs and from each other");
  if (h < 1 || w < 1 || d < 1) return fail(AMX_ERR_SHAPE, "non-positive shape (%d, %d, %d)", h, w, d);
  if (iterations < 0 || iterations > 10000) return fail(AMX_ERR_INVALID, "iterations in [0, 10000] (got %d)", iterations);
  if (int rc = amx::need_scratch(amx::ic_scratch_bytes(h, w, d), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_inverse_consistency(d_field1, d_field2, h, w, d, iterations, d_out1, d_out2, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

int amx_resize_trilinear3d(const float* d_in, int c, int h, int w, int d, float* d_out, int H, int W, int D, const float* scale,
                           int flip_channels, void* stream) {
  if (!d_in || !d_out || d_in == d_out) return fail(AMX_ERR_INVALID, "null or aliased argument");
  if (c < 1 || c > amx::kResizeMaxC) return fail(AMX_ERR_INVALID, "1 <= c <= %d (got %d)", amx::kResizeMaxC, c);
  if (h < 1 || w < 1 || d < 1 || H < 1 || W < 1 || D < 1) return fail(AMX_ERR_SHAPE, "non-positive shape");
  AMX_HIP(amx::launch_resize_trilinear(d_in, c, h, w, d, d_out, H, W, D, scale, flip_channels != 0, (hipStream_t)stream));
  return AMX_OK;
}

size_t amx_stage1_registration_scratch_bytes(int h, int w, int d, int disp_hw, int ic) {
  return (h < 1 || w < 1 || d < 1 || disp_hw < 1 || disp_hw > 3) ? 0 : amx::stage1_scratch_bytes(h, w, d, disp_hw, ic != 0);
}

int amx_stage1_registration(const float* d_feat_fix, const float* d_feat_mov, int n_ch, int h, int w, int d, int disp_hw,
                            int grid_sp, int ic, int H, int W, int D, float* d_disp_out, void* d_scratch, size_t scratch_bytes,
                            void* stream) {
  if (!d_feat_fix || !d_feat_mov || !d_disp_out || !d_scratch || n_ch < 1) return fail(AMX_ERR_INVALID, "bad argument");
  if (int rc = grid_check(h, w, d, disp_hw)) return rc;
  if (grid_sp < 1) return fail(AMX_ERR_INVALID, "grid_sp >= 1 (got %d)", grid_sp);
  if (ic && (H < 1 || W < 1 || D < 1)) return fail(AMX_ERR_SHAPE, "non-positive output shape (%d, %d, %d)", H, W, D);
  if (ic && (h < 2 || w < 2 || d < 2)) return fail(AMX_ERR_SHAPE, "inverse consistency needs a grid of at least 2 per axis");
  if (int rc = amx::need_scratch(amx::stage1_scratch_bytes(h, w, d, disp_hw, ic != 0), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_stage1(d_feat_fix, d_feat_mov, n_ch, h, w, d, disp_hw, grid_sp, ic != 0, H, W, D, d_disp_out, d_scratch,
                             (hipStream_t)stream));
  return AMX_OK;
}

}  // extern "C"
