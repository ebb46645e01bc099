// anatomix_amd -- the PrimusV2 patch decoder on SAMPLED rows, forward and backward, all fp32.
// PatchDecode is three ConvTranspose3d(k = 2, s = 2) with a channel LayerNorm + erf-GELU between them: kernel == stride, so an output
// voxel (z, y, x) has exactly one parent per stage and is a three-layer MLP on the embedding of token ((z>>3) gh + (y>>3)) gw + (x>>3);
// stage s = 1, 2, 3 takes the weight slice W_s[:, :, kz, ky, kx] with (kz, ky, kx) = bit (3 - s) of (z, y, x).  Contrastive pretraining
// reads P voxels per view of the decoded volume (PatchSampleF): these entries compute those rows [N][P][C] and their gradients and
// never form the volume.
//
// Rows are r = n P + p; the coordinates are shared by the N views.  Passes of a call (every launch on the caller's stream, no host
// read-back, no atomics on floats, every sum in one fixed order -> bit-identical run to run):
//   dr_keys      clamped coordinates -> token index tok[p] and the three stage offsets koff[s][p] in 0..7
//   dr_group     per stage the coordinates grouped by offset: perm[s][.] lists p in ascending order inside each group, gstart[s][0..8]
//   dr_pack      W_s [cin][cout][8] -> slices Wp_s [8][cin][cout] (cout contiguous: a workgroup streams ONE slice for a tile of rows)
//   dr_gemm      a tile of 32 rows of one offset group x 64 columns: out[r][j] = bias[j] + sum_k A[r][k] B[k][j], k ascending in steps of
//                16 (a step's products are added first, then the step to the running sum: the rounding error of a 1056-term sum grows
//                like that of a 66-term one), operands staged through LDS; <TRANSB> reads the slice transposed (the data gradient dh = da W^T)
//   dr_ln        one wave per row: LayerNorm over the channels (two-pass mean / variance, butterfly sums) + optional affine + erf-GELU
//   dr_ln_bwd    its adjoint per row, and the per-row terms of the affine gradients
//   dr_colsum    column sums over all rows: wave w adds rows w, w + 4, ... (16 at a time), the four sums are added in wave order
//   dr_wgrad     dW_s[:, :, k] tile = sum over the rows of offset group k (views outer, group order inner) of h^T da; a group without
//                rows stores exact zeros
//   dr_tokens    d_tokens[n][t] = sum of the stage-1 data-gradient rows whose token is t, p ascending; exact zeros where no row points
// The backward re-runs the forward passes into the scratch (one third of its arithmetic): a call reads nothing that an earlier call left
// there, which is the rule of the training scratch the ViT's other autograd entries share.
#include "amx_launch.h"

namespace amx {

namespace {

constexpr int kDrMaxE = 1056, kDrMaxC = 64;      // PrimusV2-L's embedding; the widest head the rows are computed for
constexpr int kDrMaxRows = 1 << 20;
constexpr int kDrTR = 32, kDrTC = 64, kDrTK = 16; // dr_gemm tile: rows x columns, k step
constexpr int kDrWM = 32;                        // dr_wgrad tile: input features (x kDrTC output features)

inline size_t dr_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct DrShape {
  int n, p, gd, gh, gw, e, c1, c2, c;
};

struct DrPlan {
  size_t tok, koff, perm, gstart, wp1, wp2, wp3, a1, h1, a2, h2, a3, st1, st2, st3;      // forward
  size_t g3, dh2, da2, dh1, da1, dh0, gx, gy;                                              // backward
  size_t bytes;
};

bool dr_sizes_ok(int n, int p, int e, int c1, int c2, int c) {
  return n >= 1 && n <= 65535 && p >= 1 && (long long)n * p <= kDrMaxRows && e >= 1 && e <= kDrMaxE && c1 >= 1 && c1 <= kDrMaxE && c2 >= 1 &&
         c2 <= kDrMaxE && c >= 1 && c <= kDrMaxC;
}

bool dr_plan(int n, int p, int e, int c1, int c2, int c, DrPlan* out) {
  if (!dr_sizes_ok(n, p, e, c1, c2, c)) return false;
  const size_t R = (size_t)n * p;
  const int cm = c1 > c2 ? (c1 > c ? c1 : c) : (c2 > c ? c2 : c);
  DrPlan q{};
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += dr_up(bytes); return at; };
  q.tok = take((size_t)p * 4); q.koff = take((size_t)3 * p * 4); q.perm = take((size_t)3 * p * 4); q.gstart = take(3 * 16 * 4);
  q.wp1 = take((size_t)8 * e * c1 * 4); q.wp2 = take((size_t)8 * c1 * c2 * 4); q.wp3 = take((size_t)8 * c2 * c * 4);
  q.a1 = take(R * c1 * 4); q.h1 = take(R * c1 * 4); q.a2 = take(R * c2 * 4); q.h2 = take(R * c2 * 4); q.a3 = take(R * c * 4);
  q.st1 = take(R * 8); q.st2 = take(R * 8); q.st3 = take(R * 8);
  q.g3 = take(R * c * 4); q.dh2 = take(R * c2 * 4); q.da2 = take(R * c2 * 4); q.dh1 = take(R * c1 * 4); q.da1 = take(R * c1 * 4);
  q.dh0 = take(R * e * 4); q.gx = take(R * cm * 4); q.gy = take(R * cm * 4);
  q.bytes = o;
  *out = q;
  return true;
}

__device__ __forceinline__ int dr_clamp(long long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

// grid ceil(P / 256), block 256.  Any coordinate value is clamped into the volume: no later pass can index outside its buffers.
__global__ __launch_bounds__(256) void dr_keys_kernel(const long long* __restrict__ coords, int P, int gd, int gh, int gw, int* __restrict__ tok,
                                                      int* __restrict__ koff) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int z = dr_clamp(coords[3 * (long long)p], 8 * gd - 1), y = dr_clamp(coords[3 * (long long)p + 1], 8 * gh - 1),
            x = dr_clamp(coords[3 * (long long)p + 2], 8 * gw - 1);
  tok[p] = ((z >> 3) * gh + (y >> 3)) * gw + (x >> 3);
#pragma unroll
  for (int s = 0; s < 3; ++s) koff[s * P + p] = (((z >> (2 - s)) & 1) << 2) | (((y >> (2 - s)) & 1) << 1) | ((x >> (2 - s)) & 1);
}

// one workgroup of 64: thread (s, k), s < 3, k < 8, owns offset group k of stage s: counts it, then lists its p in ascending order
__global__ __launch_bounds__(64) void dr_group_kernel(const int* __restrict__ koff, int P, int* __restrict__ perm, int* __restrict__ gstart) {
  __shared__ int cnt[24];
  const int tid = threadIdx.x, s = tid >> 3, k = tid & 7;
  if (tid < 24) {
    int c = 0;
    for (int p = 0; p < P; ++p) c += koff[s * P + p] == k;
    cnt[tid] = c;
  }
  __syncthreads();
  if (tid >= 24) return;
  int at = 0;
  for (int j = 0; j < k; ++j) at += cnt[s * 8 + j];
  gstart[s * 16 + k] = at;
  if (k == 7) gstart[s * 16 + 8] = at + cnt[tid];
  for (int p = 0; p < P; ++p)
    if (koff[s * P + p] == k) perm[s * P + at++] = p;
}

// W [pairs = cin cout][8] -> Wp [8][pairs]: a thread reads the eight offsets of one (ci, co), the stores are coalesced per offset
__global__ __launch_bounds__(256) void dr_pack_kernel(const float* __restrict__ w, long long pairs, float* __restrict__ wp) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= pairs) return;
  float v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = w[i * 8 + k];
#pragma unroll
  for (int k = 0; k < 8; ++k) wp[k * pairs + i] = v[k];
}

// tile index -> (offset group, first list position); false behind the last tile (uniform per workgroup)
__device__ __forceinline__ bool dr_tile(const int* __restrict__ gs, int t, int* k_out, int* j0, int* j1) {
  for (int k = 0; k < 8; ++k) {
    const int b = gs[k], e = gs[k + 1], nt = (e - b + kDrTR - 1) / kDrTR;
    if (t < nt) { *k_out = k; *j0 = b + t * kDrTR; *j1 = e; return true; }
    t -= nt;
  }
  return false;
}

// out[n P + p][j] = bias[j] + sum_kk A(n, p)[kk] B_k[kk][j] for the rows p of one offset group k.  A(n, p) = a + n a_view + (rowmap ?
// rowmap[p] : p) lda.  B_k = wp + k K ncols, element (kk, j) at kk ncols + j, or at j K + kk when TRANSB.
// grid (ceil(P / 32) + 8, ceil(ncols / 64), N), block 256: thread (tx, ty) owns rows 2 ty, 2 ty + 1 x columns 4 tx .. 4 tx + 3
template <bool TRANSB>
__global__ __launch_bounds__(256) void dr_gemm_kernel(const float* __restrict__ a, long long a_view, int lda, const int* __restrict__ rowmap,
                                                      const float* __restrict__ wp, int K, int ncols, const float* __restrict__ bias,
                                                      float* __restrict__ out, int P, const int* __restrict__ perm, const int* __restrict__ gs) {
  __shared__ float As[kDrTK][kDrTR + 1];
  __shared__ float Bs[kDrTK][kDrTC + 1];
  __shared__ int rows_p[kDrTR];
  int k, j0, j1;
  if (!dr_tile(gs, blockIdx.x, &k, &j0, &j1)) return;
  const int tid = threadIdx.x, n = blockIdx.z, col0 = blockIdx.y * kDrTC;
  if (tid < kDrTR) {
    int p = j0 + tid < j1 ? perm[j0 + tid] : -1;
    if (p >= P) p = -1;
    rows_p[tid] = p;
  }
  __syncthreads();
  const float* B = wp + (long long)k * K * ncols;
  const int ar = tid >> 3, ak = (tid & 7) * 2;
  const int ap = rows_p[ar];
  const float* arow = ap >= 0 ? a + n * a_view + (long long)(rowmap ? rowmap[ap] : ap) * lda : nullptr;
  const int tx = tid & 15, ty = tid >> 4;
  float acc[2][4] = {};
  for (int k0 = 0; k0 < K; k0 += kDrTK) {
#pragma unroll
    for (int i = 0; i < 2; ++i) As[ak + i][ar] = (arow && k0 + ak + i < K) ? arow[k0 + ak + i] : 0.f;
    if (!TRANSB) {
      const int kk = tid >> 4, c4 = (tid & 15) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int col = col0 + c4 + i;
        Bs[kk][c4 + i] = (k0 + kk < K && col < ncols) ? B[(long long)(k0 + kk) * ncols + col] : 0.f;
      }
    } else {
      const int kk = tid & 15, cc = tid >> 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int col = col0 + cc + 16 * i;
        Bs[kk][cc + 16 * i] = (k0 + kk < K && col < ncols) ? B[(long long)col * K + k0 + kk] : 0.f;
      }
    }
    __syncthreads();
    float part[2][4] = {};                                   // the step's 16 products first, then one addition to the running sum
#pragma unroll
    for (int kk = 0; kk < kDrTK; ++kk) {
      const float a0 = As[kk][2 * ty], a1 = As[kk][2 * ty + 1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float b = Bs[kk][4 * tx + j];
        part[0][j] = fmaf(a0, b, part[0][j]);
        part[1][j] = fmaf(a1, b, part[1][j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { acc[0][j] += part[0][j]; acc[1][j] += part[1][j]; }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = rows_p[2 * ty + i];
    if (p < 0) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = col0 + 4 * tx + j;
      if (col < ncols) out[((long long)n * P + p) * ncols + col] = acc[i][j] + (bias ? bias[col] : 0.f);
    }
  }
}

// dw[ci][co][k] = sum over views n (outer) and the rows p of offset group k (list order) of X(n, p)[ci] g[n P + p][co].
// grid (ceil(cin / 32), ceil(cout / 64), 8), block 256: thread (tx, ty) owns ci 2 ty, 2 ty + 1 x co 4 tx .. 4 tx + 3
__global__ __launch_bounds__(256) void dr_wgrad_kernel(const float* __restrict__ x, long long x_view, int ldx, const int* __restrict__ rowmap,
                                                       const float* __restrict__ g, int cin, int cout, int N, int P,
                                                       const int* __restrict__ perm, const int* __restrict__ gs, float* __restrict__ dw) {
  __shared__ float Xs[kDrTK][kDrWM + 1];
  __shared__ float Gs[kDrTK][kDrTC + 1];
  const int tid = threadIdx.x, k = blockIdx.z, ci0 = blockIdx.x * kDrWM, co0 = blockIdx.y * kDrTC;
  int b = gs[k], e = gs[k + 1];
  b = b < 0 ? 0 : b; e = e > P ? P : e;
  const int lr = tid >> 4, lx = (tid & 15) * 2, lg = (tid & 15) * 4;
  const int tx = tid & 15, ty = tid >> 4;
  float acc[2][4] = {};
  for (int n = 0; n < N; ++n)
    for (int j0 = b; j0 < e; j0 += kDrTK) {
      int p = j0 + lr < e ? perm[j0 + lr] : -1;
      if (p >= P) p = -1;
      const float* xr = p >= 0 ? x + n * x_view + (long long)(rowmap ? rowmap[p] : p) * ldx : nullptr;
      const float* gr = p >= 0 ? g + ((long long)n * P + p) * cout : nullptr;
#pragma unroll
      for (int i = 0; i < 2; ++i) Xs[lr][lx + i] = (xr && ci0 + lx + i < cin) ? xr[ci0 + lx + i] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) Gs[lr][lg + i] = (gr && co0 + lg + i < cout) ? gr[co0 + lg + i] : 0.f;
      __syncthreads();
      float part[2][4] = {};                                 // 16 rows first, then one addition to the running sum
#pragma unroll
      for (int r = 0; r < kDrTK; ++r) {
        const float x0 = Xs[r][2 * ty], x1 = Xs[r][2 * ty + 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gv = Gs[r][4 * tx + j];
          part[0][j] = fmaf(x0, gv, part[0][j]);
          part[1][j] = fmaf(x1, gv, part[1][j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) { acc[0][j] += part[0][j]; acc[1][j] += part[1][j]; }
      __syncthreads();
    }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ci = ci0 + 2 * ty + i;
    if (ci >= cin) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = co0 + 4 * tx + j;
      if (co < cout) dw[((long long)ci * cout + co) * 8 + k] = acc[i][j];
    }
  }
}

__device__ __forceinline__ float dr_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// out[r] = act(w (a[r] - mean) rstd + b) over the C channels of row r, st[r] = {mean, rstd}; w / b may be null (no affine).
// grid ceil(R / 4), block 256: one wave per row
__global__ __launch_bounds__(256) void dr_ln_kernel(const float* __restrict__ a, long long R, int C, const float* __restrict__ w,
                                                    const float* __restrict__ b, float eps, int gelu, float* __restrict__ out,
                                                    float* __restrict__ st) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;                                        // (wave-uniform; no barrier in this kernel)
  const float* row = a + r * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += row[c];
  const float mean = dr_wave_sum(s) / (float)C;
  float v = 0.f;
  for (int c = lane; c < C; c += 64) { const float d = row[c] - mean; v = fmaf(d, d, v); }
  const float rstd = 1.f / sqrtf(dr_wave_sum(v) / (float)C + eps);
  for (int c = lane; c < C; c += 64) {
    float y = (row[c] - mean) * rstd;
    if (w) y = fmaf(y, w[c], b ? b[c] : 0.f);
    out[r * C + c] = gelu ? 0.5f * y * (1.f + erff(y * 0.70710678118654752f)) : y;
  }
  if (lane == 0) { st[2 * r] = mean; st[2 * r + 1] = rstd; }
}

// adjoint of dr_ln for row r: da from dout (the gradient of the row's output); gy = d(pre-activation), gx = gy xhat -- the per-row terms of
// the affine bias / weight gradients (null: not stored).  da may alias dout.
__global__ __launch_bounds__(256) void dr_ln_bwd_kernel(const float* __restrict__ a, const float* __restrict__ st, long long R, int C,
                                                        const float* __restrict__ w, const float* __restrict__ b, int gelu,
                                                        const float* dout, float* da, float* __restrict__ gx, float* __restrict__ gy) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const float mean = st[2 * r], rstd = st[2 * r + 1];
  const float* row = a + r * C;
  auto dxhat = [&](int c, float* xh_out, float* dy_out) {
    const float xh = (row[c] - mean) * rstd;
    float dy = dout[r * C + c];
    if (gelu) {
      const float y = w ? fmaf(xh, w[c], b ? b[c] : 0.f) : xh;
      dy *= 0.5f * (1.f + erff(y * 0.70710678118654752f)) + y * 0.39894228040143268f * expf(-0.5f * y * y);
    }
    *xh_out = xh; *dy_out = dy;
    return w ? dy * w[c] : dy;
  };
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < C; c += 64) {
    float xh, dy;
    const float d = dxhat(c, &xh, &dy);
    s1 += d; s2 = fmaf(d, xh, s2);
    if (gy) gy[r * C + c] = dy;
    if (gx) gx[r * C + c] = dy * xh;
  }
  const float m1 = dr_wave_sum(s1) / (float)C, m2 = dr_wave_sum(s2) / (float)C;
  for (int c = lane; c < C; c += 64) {
    float xh, dy;
    const float d = dxhat(c, &xh, &dy);
    da[r * C + c] = rstd * (d - m1 - xh * m2);
  }
}

// dst[c] = sum over the R rows of src[r][c].  grid ceil(C / 64), block 256: wave w adds rows w, w + 4, ..., then the waves in order
__global__ __launch_bounds__(256) void dr_colsum_kernel(const float* __restrict__ src, long long R, int C, float* __restrict__ dst) {
  __shared__ float ps[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (c < C)
    for (long long r0 = wave; r0 < R; r0 += 64) {            // 16 of the wave's rows first, then one addition to the running sum
      float t = 0.f;
      for (long long r = r0; r < r0 + 64 && r < R; r += 4) t += src[r * C + c];
      s += t;
    }
  ps[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < C) dst[c] = ((ps[0][lane] + ps[1][lane]) + ps[2][lane]) + ps[3][lane];
}

// dtok[n][t][:] = sum over p ascending with tok[p] == t of dh0[n P + p][:].  grid T, block 256
__global__ __launch_bounds__(256) void dr_tokens_kernel(const float* __restrict__ dh0, const int* __restrict__ tok, int N, int P, int T, int E,
                                                        float* __restrict__ dtok) {
  const int t = blockIdx.x;
  for (int n = 0; n < N; ++n)
    for (int e = threadIdx.x; e < E; e += 256) {
      float s = 0.f, part = 0.f;                               // 16 rows first, then one addition to the running sum
      int cnt = 0;
      for (int p = 0; p < P; ++p)
        if (tok[p] == t) {
          part += dh0[((long long)n * P + p) * E + e];
          if (++cnt == 16) { s += part; part = 0.f; cnt = 0; }
        }
      dtok[((long long)n * T + t) * E + e] = s + part;
    }
}

// the twelve parameter tensors of the decoder (+ output norm) in the order of the C ABI's `params` / `grads` arrays
enum { W1, B1, LW1, LB1, W2, B2, LW2, LB2, W3, B3, OW, OB, kDrParams };

struct DrCall {
  DrShape s;
  DrPlan q;
  const float* tokens;
  const long long* coords;
  const float* prm[kDrParams];
  float ln_eps, out_eps;
  int out_norm;
  char* sc;
  hipStream_t st;
  template <typename T> T* at(size_t off) const { return (T*)(sc + off); }
  const int* perm(int stage) const { return at<int>(q.perm) + (size_t)stage * s.p; }
  const int* gs(int stage) const { return at<int>(q.gstart) + stage * 16; }
  long long rows() const { return (long long)s.n * s.p; }
};

#define DR_LAUNCHED()                                   \
  do {                                                  \
    hipError_t e_ = hipGetLastError();                  \
    if (e_ != hipSuccess) return e_;                    \
  } while (0)

template <bool TRANSB>
hipError_t dr_gemm(const DrCall& c, int stage, const float* a, long long a_view, int lda, const int* rowmap, const float* wp, int K, int ncols,
                   const float* bias, float* out) {
  hipLaunchKernelGGL((dr_gemm_kernel<TRANSB>), dim3(cdiv(c.s.p, kDrTR) + 8, cdiv(ncols, kDrTC), c.s.n), dim3(256), 0, c.st, a, a_view, lda, rowmap,
                     wp, K, ncols, bias, out, c.s.p, c.perm(stage), c.gs(stage));
  return hipGetLastError();
}

hipError_t dr_ln(const DrCall& c, const float* a, int C, const float* w, const float* b, float eps, int gelu, float* out, float* st) {
  hipLaunchKernelGGL(dr_ln_kernel, dim3(cdiv(c.rows(), 4)), dim3(256), 0, c.st, a, c.rows(), C, w, b, eps, gelu, out, st);
  return hipGetLastError();
}

hipError_t dr_ln_bwd(const DrCall& c, const float* a, const float* st, int C, const float* w, const float* b, int gelu, const float* dout,
                     float* da, float* gx, float* gy) {
  hipLaunchKernelGGL(dr_ln_bwd_kernel, dim3(cdiv(c.rows(), 4)), dim3(256), 0, c.st, a, st, c.rows(), C, w, b, gelu, dout, da, gx, gy);
  return hipGetLastError();
}

hipError_t dr_colsum(const DrCall& c, const float* src, int C, float* dst) {
  hipLaunchKernelGGL(dr_colsum_kernel, dim3(cdiv(C, 64)), dim3(256), 0, c.st, src, c.rows(), C, dst);
  return hipGetLastError();
}

hipError_t dr_wgrad(const DrCall& c, int stage, const float* x, long long x_view, int ldx, const int* rowmap, const float* g, int cin, int cout,
                    float* dw) {
  hipLaunchKernelGGL(dr_wgrad_kernel, dim3(cdiv(cin, kDrWM), cdiv(cout, kDrTC), 8), dim3(256), 0, c.st, x, x_view, ldx, rowmap, g, cin, cout, c.s.n,
                     c.s.p, c.perm(stage), c.gs(stage), dw);
  return hipGetLastError();
}

#define DR_TRY(expr)                          \
  do {                                        \
    hipError_t e_ = (expr);                   \
    if (e_ != hipSuccess) return e_;          \
  } while (0)

// keys, grouping, slices, the three stages; `rows`: where the final rows go (the a3 scratch when the backward re-runs the passes)
hipError_t dr_forward(const DrCall& c, float* rows) {
  const DrShape& s = c.s;
  const DrPlan& q = c.q;
  int* tok = c.at<int>(q.tok);
  int* koff = c.at<int>(q.koff);
  hipLaunchKernelGGL(dr_keys_kernel, dim3(cdiv(s.p, 256)), dim3(256), 0, c.st, c.coords, s.p, s.gd, s.gh, s.gw, tok, koff);
  DR_LAUNCHED();
  hipLaunchKernelGGL(dr_group_kernel, dim3(1), dim3(64), 0, c.st, koff, s.p, c.at<int>(q.perm), c.at<int>(q.gstart));
  DR_LAUNCHED();
  const int cin[3] = {s.e, s.c1, s.c2}, cout[3] = {s.c1, s.c2, s.c};
  const size_t wp[3] = {q.wp1, q.wp2, q.wp3};
  const int wi[3] = {W1, W2, W3};
  for (int i = 0; i < 3; ++i) {
    const long long pairs = (long long)cin[i] * cout[i];
    hipLaunchKernelGGL(dr_pack_kernel, dim3(cdiv(pairs, 256)), dim3(256), 0, c.st, c.prm[wi[i]], pairs, c.at<float>(wp[i]));
    DR_LAUNCHED();
  }
  const long long T = (long long)s.gd * s.gh * s.gw;
  float *a1 = c.at<float>(q.a1), *h1 = c.at<float>(q.h1), *a2 = c.at<float>(q.a2), *h2 = c.at<float>(q.h2), *a3 = c.at<float>(q.a3);
  DR_TRY(dr_gemm<false>(c, 0, c.tokens, T * s.e, s.e, tok, c.at<float>(q.wp1), s.e, s.c1, c.prm[B1], a1));
  DR_TRY(dr_ln(c, a1, s.c1, c.prm[LW1], c.prm[LB1], c.ln_eps, 1, h1, c.at<float>(q.st1)));
  DR_TRY(dr_gemm<false>(c, 1, h1, (long long)s.p * s.c1, s.c1, nullptr, c.at<float>(q.wp2), s.c1, s.c2, c.prm[B2], a2));
  DR_TRY(dr_ln(c, a2, s.c2, c.prm[LW2], c.prm[LB2], c.ln_eps, 1, h2, c.at<float>(q.st2)));
  float* last = c.out_norm ? a3 : rows;
  DR_TRY(dr_gemm<false>(c, 2, h2, (long long)s.p * s.c2, s.c2, nullptr, c.at<float>(q.wp3), s.c2, s.c, c.prm[B3], last));
  if (c.out_norm) DR_TRY(dr_ln(c, a3, s.c, c.prm[OW], c.prm[OB], c.out_eps, 0, rows, c.at<float>(q.st3)));
  return hipSuccess;
}

hipError_t dr_backward(const DrCall& c, const float* drows, float* dtokens, float* const* g) {
  const DrShape& s = c.s;
  const DrPlan& q = c.q;
  // with an output norm the re-run's normalised rows are not needed: they go where g3 is written afterwards
  DR_TRY(dr_forward(c, c.out_norm ? c.at<float>(q.g3) : c.at<float>(q.a3)));
  const int* tok = c.at<int>(q.tok);
  float *gx = c.at<float>(q.gx), *gy = c.at<float>(q.gy);
  const float* g3 = drows;
  if (c.out_norm) {
    const bool affine = c.prm[OW] != nullptr;
    DR_TRY(dr_ln_bwd(c, c.at<float>(q.a3), c.at<float>(q.st3), s.c, c.prm[OW], c.prm[OB], 0, drows, c.at<float>(q.g3), affine ? gx : nullptr,
                     affine ? gy : nullptr));
    if (affine && g[OW]) DR_TRY(dr_colsum(c, gx, s.c, g[OW]));
    if (affine && g[OB]) DR_TRY(dr_colsum(c, gy, s.c, g[OB]));
    g3 = c.at<float>(q.g3);
  }
  const float *h1 = c.at<float>(q.h1), *h2 = c.at<float>(q.h2);
  float *dh2 = c.at<float>(q.dh2), *da2 = c.at<float>(q.da2), *dh1 = c.at<float>(q.dh1), *da1 = c.at<float>(q.da1), *dh0 = c.at<float>(q.dh0);
  // stage 3
  if (g[B3]) DR_TRY(dr_colsum(c, g3, s.c, g[B3]));
  if (g[W3]) DR_TRY(dr_wgrad(c, 2, h2, (long long)s.p * s.c2, s.c2, nullptr, g3, s.c2, s.c, g[W3]));
  DR_TRY(dr_gemm<true>(c, 2, g3, (long long)s.p * s.c, s.c, nullptr, c.at<float>(q.wp3), s.c, s.c2, nullptr, dh2));
  // stage 2
  DR_TRY(dr_ln_bwd(c, c.at<float>(q.a2), c.at<float>(q.st2), s.c2, c.prm[LW2], c.prm[LB2], 1, dh2, da2, gx, gy));
  if (g[LW2]) DR_TRY(dr_colsum(c, gx, s.c2, g[LW2]));
  if (g[LB2]) DR_TRY(dr_colsum(c, gy, s.c2, g[LB2]));
  if (g[B2]) DR_TRY(dr_colsum(c, da2, s.c2, g[B2]));
  if (g[W2]) DR_TRY(dr_wgrad(c, 1, h1, (long long)s.p * s.c1, s.c1, nullptr, da2, s.c1, s.c2, g[W2]));
  DR_TRY(dr_gemm<true>(c, 1, da2, (long long)s.p * s.c2, s.c2, nullptr, c.at<float>(q.wp2), s.c2, s.c1, nullptr, dh1));
  // stage 1
  DR_TRY(dr_ln_bwd(c, c.at<float>(q.a1), c.at<float>(q.st1), s.c1, c.prm[LW1], c.prm[LB1], 1, dh1, da1, gx, gy));
  if (g[LW1]) DR_TRY(dr_colsum(c, gx, s.c1, g[LW1]));
  if (g[LB1]) DR_TRY(dr_colsum(c, gy, s.c1, g[LB1]));
  if (g[B1]) DR_TRY(dr_colsum(c, da1, s.c1, g[B1]));
  const long long T = (long long)s.gd * s.gh * s.gw;
  if (g[W1]) DR_TRY(dr_wgrad(c, 0, c.tokens, T * s.e, s.e, tok, da1, s.e, s.c1, g[W1]));
  if (dtokens) {
    DR_TRY(dr_gemm<true>(c, 0, da1, (long long)s.p * s.c1, s.c1, nullptr, c.at<float>(q.wp1), s.c1, s.e, nullptr, dh0));
    hipLaunchKernelGGL(dr_tokens_kernel, dim3((unsigned)T), dim3(256), 0, c.st, dh0, tok, s.n, s.p, (int)T, s.e, dtokens);
    DR_LAUNCHED();
  }
  return hipSuccess;
}

// the checks both entries share: AMX_OK and a filled call, or the refusal -- before any launch
int dr_prepare(const char* what, const float* d_tokens, const long long* d_coords, const void* const* params, int n, int p, int gd, int gh, int gw,
               int e, int c1, int c2, int c, float ln_eps, int out_norm, float out_eps, void* d_scratch, size_t scratch_bytes, void* stream,
               DrCall* call) {
  if (!d_tokens || !d_coords || !params) return fail(AMX_ERR_INVALID, "%s: null argument", what);
  DrCall k{};
  if (!dr_plan(n, p, e, c1, c2, c, &k.q) || gd < 1 || gh < 1 || gw < 1 || (long long)gd * gh * gw > (1 << 24))
    return fail(AMX_ERR_SHAPE,
                "%s: views %d, rows %d, token grid (%d, %d, %d), widths %d / %d / %d / %d are outside the envelope (patch 8; widths up to %d, "
                "output channels up to %d, views x rows up to 2^20, tokens up to 2^24)",
                what, n, p, gd, gh, gw, e, c1, c2, c, kDrMaxE, kDrMaxC);
  if (out_norm < 0 || out_norm > 2) return fail(AMX_ERR_INVALID, "%s: out_norm is 0 (none), 1 (layernorm) or 2 (layernorm_affine), got %d", what, out_norm);
  for (int i = 0; i < kDrParams; ++i) k.prm[i] = (const float*)params[i];
  const int must[] = {W1, LW1, LB1, W2, LW2, LB2, W3};
  for (int i : must)
    if (!k.prm[i]) return fail(AMX_ERR_INVALID, "%s: params[%d] is null (only the conv biases and the output norm's pair may be)", what, i);
  if (out_norm == 2 && !(k.prm[OW] && k.prm[OB])) return fail(AMX_ERR_INVALID, "%s: layernorm_affine needs params[10] and params[11]", what);
  if (out_norm != 2) k.prm[OW] = k.prm[OB] = nullptr;
  if (!d_scratch || scratch_bytes < k.q.bytes || ((uintptr_t)d_scratch & 15))
    return fail(AMX_ERR_WORKSPACE, "%s scratch needs %zu bytes, 16-byte aligned", what, k.q.bytes);
  k.s = DrShape{n, p, gd, gh, gw, e, c1, c2, c};
  k.tokens = d_tokens; k.coords = d_coords; k.ln_eps = ln_eps; k.out_eps = out_eps; k.out_norm = out_norm;
  k.sc = (char*)d_scratch; k.st = (hipStream_t)stream;
  *call = k;
  return AMX_OK;
}

}  // namespace

}  // namespace amx

extern "C" {

size_t amx_vit_decode_rows_scratch_bytes(int n, int p, int e, int c1, int c2, int c) {
  amx::DrPlan q;
  return amx::dr_plan(n, p, e, c1, c2, c, &q) ? q.bytes : 0;
}

int amx_vit_decode_rows_forward(const float* d_tokens, const long long* d_coords, const void* const* params, int n, int p, int gd, int gh, int gw,
                                int e, int c1, int c2, int c, float ln_eps, int out_norm, float out_eps, float* d_rows, void* d_scratch,
                                size_t scratch_bytes, void* stream) {
  amx::DrCall call;
  if (int rc = amx::dr_prepare("decode rows forward", d_tokens, d_coords, params, n, p, gd, gh, gw, e, c1, c2, c, ln_eps, out_norm, out_eps, d_scratch,
                               scratch_bytes, stream, &call))
    return rc;
  if (!d_rows) return amx::fail(AMX_ERR_INVALID, "decode rows forward: null d_rows");
  AMX_HIP(amx::dr_forward(call, d_rows));
  return AMX_OK;
}

int amx_vit_decode_rows_backward(const float* d_tokens, const long long* d_coords, const void* const* params, int n, int p, int gd, int gh, int gw,
                                 int e, int c1, int c2, int c, float ln_eps, int out_norm, float out_eps, const float* d_drows, float* d_dtokens,
                                 void* const* grads, void* d_scratch, size_t scratch_bytes, void* stream) {
  amx::DrCall call;
  if (int rc = amx::dr_prepare("decode rows backward", d_tokens, d_coords, params, n, p, gd, gh, gw, e, c1, c2, c, ln_eps, out_norm, out_eps,
                               d_scratch, scratch_bytes, stream, &call))
    return rc;
  if (!d_drows || !grads) return amx::fail(AMX_ERR_INVALID, "decode rows backward: null argument");
  float* g[amx::kDrParams];
  for (int i = 0; i < amx::kDrParams; ++i) g[i] = (float*)grads[i];
  AMX_HIP(amx::dr_backward(call, d_drows, d_dtokens, g));
  return AMX_OK;
}

}  // extern "C"
