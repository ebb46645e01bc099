// anatomix_amd -- the token LayerNorms of an EVA block under autograd, optionally fed by the SwiGLU gate: for fp32 x [M][C] (and gate
// [M][C]), w, b [C]
//   u = x                     (plain: norm1, attn.norm, norm2, the final norm)
//   u = silu(gate) * x        (gated: mlp.norm, the widest tensors of the network)
//   y = (u - mean) * rstd * w + b,    mean = mean_c(u),  rstd = 1 / sqrt(mean_c((u - mean)^2) + eps)          (nn.LayerNorm)
// and the gradients, with x^ = (u - mean) * rstd recomputed from x (and gate), mean and rstd, t = dy * w:
//   du = rstd * (t - mean_c(t) - x^ * mean_c(t * x^))        dw = sum_rows dy * x^        db = sum_rows dy
//   plain:  dx = du          gated, s = sigmoid(gate):  dx = du * gate * s,   dgate = du * x * s * (1 + gate * (1 - s))
// A wave owns whole rows and keeps them in registers: lane l holds the quads l, l + 64, ... of a row (NQ quads, 16-byte loads and stores;
// NQ = 16 covers C = 4096), so a row is read once and u is never stored.  Row sums are wave reductions (xor butterfly: every lane ends with
// the same bits); the statistics are two-pass (the mean, then the variance of the deviations) like the project's other norm kernels.
// Passes:
//   forward    ln_fwd<NQ, GATED>   one row per wave, grid ceil(M / 4)
//   backward   ln_bwd<NQ, GATED>   a wave walks `rpw` rows (rows 4 i + wave of its workgroup's block of 4 rpw rows) and sums dy * x^ and dy in
//                                  registers; the four waves' sums are added in wave order through LDS and stored as the workgroup's
//                                  partial [workgroup][C] in the scratch
//              ln_fold             dw / db = the partials added in one fixed order
// The grid is a function of (M, C) alone and there are no atomics: results are bit-identical run to run.  A null output skips its
// work (no row reductions without dx / dgate, no partials and no fold without dw / db); the code of the other outputs is the same
// instructions either way, so their bits do not change.
#include "amx_launch.h"

namespace amx {

namespace {

constexpr int kLnMaxC = 4096;
constexpr int kLnRowsPerWave = 4;        // rows per wave of ln_bwd, at least
constexpr int kLnMaxWg = 512;            // workgroups (= partials) of ln_bwd, at most

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct LnPlan {
  int nq;              // quads per lane: the template instance
  int rpw, nwg;        // ln_bwd: rows per wave, workgroups
  size_t part_w, part_b, bytes;
};

bool ln_plan(long long M, int C, LnPlan* out) {
  if (M < 1 || C < 8 || C > kLnMaxC || (C & 3) || M * (long long)C >= (1LL << 31)) return false;
  LnPlan p{};
  const int need = cdiv(C / 4, 64);
  static const int sizes[] = {1, 2, 3, 4, 6, 8, 11, 16};
  for (int s : sizes)
    if (s >= need) { p.nq = s; break; }
  p.rpw = cdiv(M, 4LL * kLnMaxWg);
  if (p.rpw < kLnRowsPerWave) p.rpw = kLnRowsPerWave;
  p.nwg = cdiv(M, 4LL * p.rpw);
  p.part_w = 0;
  p.part_b = up256((size_t)p.nwg * C * 4);
  p.bytes = 2 * p.part_b;
  *out = p;
  return true;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float quad_sum(const float4 v) { return (v.x + v.y) + (v.z + v.w); }

// silu(g) * x of one element; s = sigmoid(g)
__device__ __forceinline__ float gate_mul(float g, float x, float& s) {
  s = 1.f / (1.f + expf(-g));
  return (g * s) * x;
}

// the two-pass statistics of a row held in u (quads behind the row are zeros and are left out of the deviations)
template <int NQ>
__device__ __forceinline__ void row_stats(const float4 (&u)[NQ], int lane, int nq, int C, float eps, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) s += quad_sum(u[q]);
  mean = wave_sum(s) / (float)C;
  float v = 0.f;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (q * 64 + lane < nq) {
      const float a = u[q].x - mean, b = u[q].y - mean, c = u[q].z - mean, d = u[q].w - mean;
      v += (a * a + b * b) + (c * c + d * d);
    }
  rstd = 1.f / sqrtf(wave_sum(v) / (float)C + eps);
}

// grid ceil(M / 4), block 256: wave `wave` of workgroup `g` owns row 4 g + wave
template <int NQ, bool GATED>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gate, const float* __restrict__ w,
                                                     const float* __restrict__ b, float eps, long long M, int C, float* __restrict__ y,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nq = C >> 2;
  const long long row = (long long)blockIdx.x * 4 + wave;
  if (row >= M) return;                                                  // (no barrier in this kernel)
  const float4* xr = (const float4*)(x + row * C);
  float4 u[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = q * 64 + lane;
    u[q] = i < nq ? xr[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (GATED) {
    const float4* gr = (const float4*)(gate + row * C);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i = q * 64 + lane;
      if (i < nq) {
        const float4 g = gr[i];
        float s;
        u[q].x = gate_mul(g.x, u[q].x, s); u[q].y = gate_mul(g.y, u[q].y, s);
        u[q].z = gate_mul(g.z, u[q].z, s); u[q].w = gate_mul(g.w, u[q].w, s);
      }
    }
  }
  float mean, rstd;
  row_stats<NQ>(u, lane, nq, C, eps, mean, rstd);
  if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
  float4* yr = (float4*)(y + row * C);
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = q * 64 + lane;
    if (i < nq) {
      const float4 wv = ((const float4*)w)[i], bv = ((const float4*)b)[i];
      yr[i] = make_float4((u[q].x - mean) * rstd * wv.x + bv.x, (u[q].y - mean) * rstd * wv.y + bv.y,
                          (u[q].z - mean) * rstd * wv.z + bv.z, (u[q].w - mean) * rstd * wv.w + bv.w);
    }
  }
}

// the gated input of four elements: u = silu(g) x and its two factors, fx = d u / d x = g s, fg = d u / d gate = x s (1 + g (1 - s))
__device__ __forceinline__ float gate_factors(float g, float x, float& fx, float& fg) {
  float s;
  const float u = gate_mul(g, x, s);
  fx = g * s;
  fg = x * s * (1.f + g * (1.f - s));
  return u;
}
__device__ __forceinline__ float4 gate_factors4(const float4 g, const float4 x, float4& fx, float4& fg) {
  return make_float4(gate_factors(g.x, x.x, fx.x, fg.x), gate_factors(g.y, x.y, fx.y, fg.y), gate_factors(g.z, x.z, fx.z, fg.z),
                     gate_factors(g.w, x.w, fx.w, fg.w));
}

// grid nwg, block 256; pw / pb: partials [nwg][C] or null.  Registers per lane, in quads: x^, dy (then t), the two sums -- and, gated, the
// two factors, which the widest instance (NQ = 16) has no room for: it reads x and gate a second time where it stores.
template <int NQ, bool GATED>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gate, const float* __restrict__ w,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ dy, long long M, int C, int rpw, float* __restrict__ dx,
                                                     float* __restrict__ dgate, float* __restrict__ pw, float* __restrict__ pb) {
  constexpr bool KEEP = GATED && NQ <= 11;
  __shared__ float4 red[2][NQ * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nq = C >> 2;
  const bool data = dx || (GATED && dgate);                               // (every flag is uniform)
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 aw[NQ], ab[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) aw[q] = ab[q] = zero;
  const long long row0 = (long long)blockIdx.x * 4 * rpw + wave;
  for (int r = 0; r < rpw; ++r) {
    const long long row = row0 + 4LL * r;
    if (row >= M) break;                                                 // (the barriers are behind the loop)
    const float4* xr = (const float4*)(x + row * C);
    const float4* gr = GATED ? (const float4*)(gate + row * C) : nullptr;
    const float4* dr = (const float4*)(dy + row * C);
    const float m = mean[row], rs = rstd[row];
    float4 xh[NQ], d[NQ], fx[KEEP ? NQ : 1], fg[KEEP ? NQ : 1];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {                                         // quads behind the row are zeros everywhere
      const int i = q * 64 + lane;
      xh[q] = d[q] = zero;
      if (i >= nq) continue;
      float4 u = xr[i];
      d[q] = dr[i];
      if constexpr (GATED) {
        float4 a, b;
        u = gate_factors4(gr[i], u, a, b);
        if constexpr (KEEP) { fx[q] = a; fg[q] = b; }
      }
      xh[q] = make_float4((u.x - m) * rs, (u.y - m) * rs, (u.z - m) * rs, (u.w - m) * rs);
    }
    if (pb) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) { ab[q].x += d[q].x; ab[q].y += d[q].y; ab[q].z += d[q].z; ab[q].w += d[q].w; }
    }
    if (pw) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        aw[q].x += d[q].x * xh[q].x; aw[q].y += d[q].y * xh[q].y; aw[q].z += d[q].z * xh[q].z; aw[q].w += d[q].w * xh[q].w;
      }
    }
    if (!data) continue;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i = q * 64 + lane;
      const float4 wv = i < nq ? ((const float4*)w)[i] : zero;
      d[q].x *= wv.x; d[q].y *= wv.y; d[q].z *= wv.z; d[q].w *= wv.w;        // t = dy w
      s1 += quad_sum(d[q]);
      s2 += (d[q].x * xh[q].x + d[q].y * xh[q].y) + (d[q].z * xh[q].z + d[q].w * xh[q].w);
    }
    const float c1 = wave_sum(s1) / (float)C, c2 = wave_sum(s2) / (float)C;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int i = q * 64 + lane;
      if (i >= nq) continue;
      const float4 du = make_float4(rs * (d[q].x - c1 - xh[q].x * c2), rs * (d[q].y - c1 - xh[q].y * c2),
                                    rs * (d[q].z - c1 - xh[q].z * c2), rs * (d[q].w - c1 - xh[q].w * c2));
      if constexpr (GATED) {
        float4 a, b;
        if constexpr (KEEP) { a = fx[q]; b = fg[q]; }
        else gate_factors4(gr[i], xr[i], a, b);
        if (dx) ((float4*)(dx + row * C))[i] = make_float4(du.x * a.x, du.y * a.y, du.z * a.z, du.w * a.w);
        if (dgate) ((float4*)(dgate + row * C))[i] = make_float4(du.x * b.x, du.y * b.y, du.z * b.z, du.w * b.w);
      } else {
        ((float4*)(dx + row * C))[i] = du;
      }
    }
  }
  if (!pw && !pb) return;                                                // (uniform)
  // the waves' sums in wave order: ((w0 + w1) + w2) + w3
  for (int v = 0; v < 4; ++v) {
    if (wave == v) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int i = q * 64 + lane;
        if (v == 0) {
          red[0][i] = aw[q]; red[1][i] = ab[q];
        } else {
          const float4 a = red[0][i], c = red[1][i];
          red[0][i] = make_float4(a.x + aw[q].x, a.y + aw[q].y, a.z + aw[q].z, a.w + aw[q].w);
          red[1][i] = make_float4(c.x + ab[q].x, c.y + ab[q].y, c.z + ab[q].z, c.w + ab[q].w);
        }
      }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < nq; i += 256) {
    if (pw) ((float4*)(pw + (long long)blockIdx.x * C))[i] = red[0][i];
    if (pb) ((float4*)(pb + (long long)blockIdx.x * C))[i] = red[1][i];
  }
}

// out[c] = the nwg partials of column c in one fixed order: wave v of a workgroup adds the partials v, v + 4, ... of its 64 columns into
// four interleaved sums, thread (0, column) adds the waves' sums in wave order.  grid (ceil(C / 64), 2), block 256; y = 0: dw, y = 1: db
__global__ __launch_bounds__(256) void ln_fold_kernel(const float* __restrict__ pw, const float* __restrict__ pb, int nwg, int C,
                                                      float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float psum[4][64];
  const float* part = blockIdx.y ? pb : pw;
  float* out = blockIdx.y ? db : dw;
  if (!out) return;                                                      // (uniform per workgroup)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    int p = wave;
    for (; p + 12 < nwg; p += 16) {
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] += part[(long long)(p + 4 * q) * C + c];
    }
    for (int q = 0; p < nwg; p += 4, ++q) a[q] += part[(long long)p * C + c];
  }
  psum[wave][lane] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  if (wave == 0 && c < C) out[c] = ((psum[0][lane] + psum[1][lane]) + psum[2][lane]) + psum[3][lane];
}

template <int NQ>
hipError_t launch_fwd_nq(const float* x, const float* gate, const float* w, const float* b, float eps, long long M, int C, float* y, float* mean,
                         float* rstd, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(M, 4)), block(256);
  if (gate) hipLaunchKernelGGL((ln_fwd_kernel<NQ, true>), grid, block, 0, st, x, gate, w, b, eps, M, C, y, mean, rstd);
  else hipLaunchKernelGGL((ln_fwd_kernel<NQ, false>), grid, block, 0, st, x, gate, w, b, eps, M, C, y, mean, rstd);
  return hipGetLastError();
}

template <int NQ>
hipError_t launch_bwd_nq(const float* x, const float* gate, const float* w, const float* mean, const float* rstd, const float* dy, long long M,
                         int C, const LnPlan& p, float* dx, float* dgate, float* pw, float* pb, hipStream_t st) {
  const dim3 grid((unsigned)p.nwg), block(256);
  if (gate) hipLaunchKernelGGL((ln_bwd_kernel<NQ, true>), grid, block, 0, st, x, gate, w, mean, rstd, dy, M, C, p.rpw, dx, dgate, pw, pb);
  else hipLaunchKernelGGL((ln_bwd_kernel<NQ, false>), grid, block, 0, st, x, gate, w, mean, rstd, dy, M, C, p.rpw, dx, dgate, pw, pb);
  return hipGetLastError();
}

#define AMX_LN_DISPATCH(nq, call, ...)             \
  switch (nq) {                                    \
    case 1: return call<1>(__VA_ARGS__);           \
    case 2: return call<2>(__VA_ARGS__);           \
    case 3: return call<3>(__VA_ARGS__);           \
    case 4: return call<4>(__VA_ARGS__);           \
    case 6: return call<6>(__VA_ARGS__);           \
    case 8: return call<8>(__VA_ARGS__);           \
    case 11: return call<11>(__VA_ARGS__);         \
    case 16: return call<16>(__VA_ARGS__);         \
    default: return hipErrorInvalidValue;          \
  }

}  // namespace

static size_t layernorm_train_scratch_bytes(long long M, int C) {
  LnPlan p;
  return ln_plan(M, C, &p) ? p.bytes : 0;
}

static hipError_t launch_layernorm_forward(const float* x, const float* gate, const float* w, const float* b, float eps, long long M, int C,
                                           float* y, float* mean, float* rstd, hipStream_t st) {
  LnPlan p;
  if (!ln_plan(M, C, &p)) return hipErrorInvalidValue;
  AMX_LN_DISPATCH(p.nq, launch_fwd_nq, x, gate, w, b, eps, M, C, y, mean, rstd, st);
}

static hipError_t launch_layernorm_backward(const float* x, const float* gate, const float* w, const float* mean, const float* rstd,
                                            const float* dy, long long M, int C, float* dx, float* dgate, float* dw, float* db, void* scratch,
                                            hipStream_t st) {
  LnPlan p;
  if (!ln_plan(M, C, &p)) return hipErrorInvalidValue;
  if (!dx && !dgate && !dw && !db) return hipSuccess;
  float* pw = dw ? (float*)((char*)scratch + p.part_w) : nullptr;
  float* pb = db ? (float*)((char*)scratch + p.part_b) : nullptr;
  auto main_pass = [&]() -> hipError_t { AMX_LN_DISPATCH(p.nq, launch_bwd_nq, x, gate, w, mean, rstd, dy, M, C, p, dx, dgate, pw, pb, st); };
  hipError_t e = main_pass();
  if (e != hipSuccess || (!dw && !db)) return e;
  hipLaunchKernelGGL(ln_fold_kernel, dim3((unsigned)cdiv(C, 64), 2), dim3(256), 0, st, (const float*)pw, (const float*)pb, p.nwg, C, dw, db);
  return hipGetLastError();
}

}  // namespace amx

namespace {
using amx::fail;

int layernorm_envelope(const char* what, long long m, int c) {
  if (amx::layernorm_train_scratch_bytes(m, c) == 0)
    return fail(AMX_ERR_INVALID, "%s: (M, C) = (%lld, %d) is outside the envelope (C a multiple of 4, 8 <= C <= 4096, M >= 1, M * C < 2^31)", what,
                m, c);
  return AMX_OK;
}
bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr,
               const void* f = nullptr) {
  return !(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e | (uintptr_t)f) & 15);
}
}  // namespace

extern "C" {

size_t amx_layernorm_train_scratch_bytes(long long m, int c) { return amx::layernorm_train_scratch_bytes(m, c); }

int amx_layernorm_train_forward(const float* d_x, const float* d_gate, const float* d_w, const float* d_b, float eps, long long m, int c,
                                float* d_y, float* d_mean, float* d_rstd, void* stream) {
  if (!d_x || !d_w || !d_b || !d_y || !d_mean || !d_rstd) return fail(AMX_ERR_INVALID, "layernorm forward: null argument");
  if (int rc = layernorm_envelope("layernorm forward", m, c)) return rc;
  if (!(eps >= 0.f)) return fail(AMX_ERR_INVALID, "layernorm forward: eps must be >= 0 (got %g)", (double)eps);
  if (!aligned16(d_x, d_gate, d_w, d_b, d_y)) return fail(AMX_ERR_INVALID, "layernorm forward: d_x, d_gate, d_w, d_b and d_y must be 16-byte aligned");
  AMX_HIP(amx::launch_layernorm_forward(d_x, d_gate, d_w, d_b, eps, m, c, d_y, d_mean, d_rstd, (hipStream_t)stream));
  return AMX_OK;
}

int amx_layernorm_backward(const float* d_x, const float* d_gate, const float* d_w, const float* d_mean, const float* d_rstd, const float* d_dy,
                           long long m, int c, float* d_dx, float* d_dgate, float* d_dw, float* d_db, void* d_scratch, size_t scratch_bytes,
                           void* stream) {
  if (!d_x || !d_w || !d_mean || !d_rstd || !d_dy) return fail(AMX_ERR_INVALID, "layernorm backward: null argument");
  if (int rc = layernorm_envelope("layernorm backward", m, c)) return rc;
  if (!d_gate && d_dgate) return fail(AMX_ERR_INVALID, "layernorm backward: d_dgate without d_gate");
  const size_t need = amx::layernorm_train_scratch_bytes(m, c);
  if (!d_scratch || scratch_bytes < need || ((uintptr_t)d_scratch & 15))
    return fail(AMX_ERR_WORKSPACE, "layernorm backward scratch needs %zu bytes, 16-byte aligned", need);
  if (!aligned16(d_x, d_gate, d_w, d_dy, d_dx, d_dgate))
    return fail(AMX_ERR_INVALID, "layernorm backward: d_x, d_gate, d_w, d_dy, d_dx and d_dgate must be 16-byte aligned");
  AMX_HIP(amx::launch_layernorm_backward(d_x, d_gate, d_w, d_mean, d_rstd, d_dy, m, c, d_dx, d_dgate, d_dw, d_db, d_scratch,
                                         (hipStream_t)stream));
  return AMX_OK;
}

}  // extern "C"
