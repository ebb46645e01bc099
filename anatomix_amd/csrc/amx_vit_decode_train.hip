// anatomix_amd -- the PrimusV2 patch decoder on the WHOLE volume under autograd, with the spatial output norms, all fp32.
// PatchDecode is three ConvTranspose3d(k = 2, s = 2) with a channel LayerNorm + erf-GELU between them.  Kernel == stride, so a stage is
// a row product [R, Cin] x [Cin, 8 Cout] whose output, read as [8 R, Cout], is the next stage's input WITHOUT moving data -- the rows
// stay in nested order: token (n T + t), then the child offset k1 = (kz, ky, kx) of stage 1, then k2 of stage 2:
//   R0 = N T rows of E;   R1 = 8 R0 rows of c1 (r1 = 8 r0 + k1);   R2 = 8 R1 rows of c2 (r2 = 8 r1 + k2);   columns of stage 3: k3 C + c
// LayerNorm and GELU are row operators of width c_s.  Only the last stage leaves the nested order: its epilogue stores planar fp32
// out[n][c][8 tz + 4 kz1 + 2 kz2 + kz3][..y..][..x..]; the backward gathers dy back into nested rows g3 [R2, 8 C].
//
// Arithmetic: every product runs on the f32-input MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products, an fmaf chain along k), so no
// operand is rounded and no gradient needs a scale; LayerNorm, GELU, their adjoints and every reduction are fp32, the per-(n, c)
// statistics are combined in double.  No atomics; a long sum goes through partials that are added in one fixed order; the grids are
// functions of the shape alone: bit-identical results run to run.
//
// Kernels (the instance is chosen by the USE, never by a size: a test at a small shape runs what a 128^3 step runs)
//   dt_pack             W [cin][cout][8] -> Bp [cin][8 cout] (forward operand) and Bt [8 cout][cin] (data-gradient operand)
//   dt_gemm<TA, EPI>    64 x 64 tile, k steps of 16 through LDS, 4 waves x (2 x 2) MFMA tiles.  <0, ROWS> out = A B + bias (stages 1, 2,
//                       every data gradient); <0, PLANAR> stage 3; <1, ROWS> dW partial = A^T G over a chunk of rows (grid.z chunks)
//   dt_ln               one wave per row, the row in registers: mean, rstd (two-pass), h = GELU(LN(a)); or h from saved mean / rstd
//   dt_ln_bwd           da from (a, mean, rstd, dh), in place; a workgroup's 128 rows give one partial of dgamma, dbeta and db
//   dt_colpart / dt_colreduce / dt_wreduce     partials -> sums, in fixed order
//   dt_plane_partial<MODE> / dt_plane_final / dt_plane_apply   per-(n, c) statistics of a planar volume and the in-place output norm
//   dt_gather           planar dy (+ the output norm's adjoint) -> nested rows g3
// The backward reads the raw a_1, a_2 and the rows' mean / rstd from `saved` (state of the autograd node) and recomputes h_1, h_2 into
// the scratch; it re-packs the weights: a call reads nothing that an earlier call left in the scratch.
#include "amx_launch.h"

namespace amx {

namespace {

constexpr int kDtMaxE = 1056, kDtMaxC1 = 328, kDtMaxC2 = 104, kDtMaxC = 128;
constexpr int kDtTM = 64, kDtTN = 64, kDtTK = 16, kDtLD = 80;      // tile; LDS row stride: the four k rows a wave reads sit 16 banks apart
constexpr int kDtLnMax = 6;                                        // row values per lane of dt_ln / dt_ln_bwd: widths up to 384
constexpr int kDtLnRows = 128;                                     // rows per workgroup of dt_ln_bwd (one partial each)
constexpr int kDtColRows = 256;                                    // rows per workgroup of dt_colpart
constexpr int kDtPlaneChunk = 8192;                                // voxels per workgroup of dt_plane_partial
constexpr long long kDtWgradRows = 1024;                           // rows per weight-gradient partial, at least
constexpr int kDtWgradMaxSplits = 512;
enum { DT_EPI_ROWS = 0, DT_EPI_PLANAR = 1 };
enum { DT_NORM_NONE = 0, DT_NORM_DEMEAN = 1, DT_NORM_INSTANCE = 2 };
// the ten parameter tensors in the order of the C ABI's `params` / `grads` arrays
enum { W1, B1, LW1, LB1, W2, B2, LW2, LB2, W3, B3, kDtParams };

typedef float f32x4 __attribute__((ext_vector_type(4)));

inline size_t dt_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct DtShape {
  int n, gd, gh, gw, e, c1, c2, c;
  long long T() const { return (long long)gd * gh * gw; }
  long long R0() const { return n * T(); }
  long long R1() const { return 8 * R0(); }
  long long R2() const { return 64 * R0(); }
  long long V() const { return 512 * T(); }      // voxels per (n, c) plane
};

struct DtPlan {
  size_t a1, a2, st1, st2, ostat, saved_bytes;                                              // saved
  size_t bp[3], bt[3], h1, h2, g3, dh2, dh1, wpart, lnpart, colpart, plpart, bstat, bytes;  // scratch
  int wsplit[3];
  long long wchunk[3];
  int nplchunk;
};

bool dt_shape_ok(const DtShape& s) {
  if (s.n < 1 || s.gd < 1 || s.gh < 1 || s.gw < 1) return false;
  if (s.e < 4 || s.e > kDtMaxE || s.c1 < 4 || s.c1 > kDtMaxC1 || s.c2 < 4 || s.c2 > kDtMaxC2 || ((s.e | s.c1 | s.c2) & 3)) return false;
  if (s.c < 1 || s.c > kDtMaxC) return false;
  const long long lim = 1LL << 31;
  const double t = (double)s.gd * s.gh * s.gw * s.n;
  if (t * 512.0 * s.c >= (double)lim || t * 64.0 * s.c2 >= (double)lim || t * 8.0 * s.c1 >= (double)lim || t * s.e >= (double)lim) return false;
  return (long long)s.n * s.c <= 65535;          // planes are grid.y
}

bool dt_plan(const DtShape& s, DtPlan* out) {
  if (!dt_shape_ok(s)) return false;
  DtPlan q{};
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += dt_up(bytes); return at; };
  const size_t R0 = s.R0(), R1 = s.R1(), R2 = s.R2();
  q.a1 = take(R1 * s.c1 * 4); q.a2 = take(R2 * s.c2 * 4); q.st1 = take(R1 * 8); q.st2 = take(R2 * 8); q.ostat = take((size_t)s.n * s.c * 8);
  q.saved_bytes = o;
  o = 0;
  const int cin[3] = {s.e, s.c1, s.c2}, cout[3] = {s.c1, s.c2, s.c};
  const size_t rows[3] = {R0, R1, R2};
  size_t wpart = 0;
  for (int i = 0; i < 3; ++i) {
    q.bp[i] = take((size_t)cin[i] * 8 * cout[i] * 4);
    q.bt[i] = take((size_t)cin[i] * 8 * cout[i] * 4);
    long long chunk = ((long long)rows[i] + kDtWgradMaxSplits - 1) / kDtWgradMaxSplits;
    chunk = (chunk + kDtTK - 1) / kDtTK * kDtTK;
    if (chunk < kDtWgradRows) chunk = kDtWgradRows;
    q.wchunk[i] = chunk;
    q.wsplit[i] = (int)(((long long)rows[i] + chunk - 1) / chunk);
    const size_t need = (size_t)q.wsplit[i] * cin[i] * 8 * cout[i] * 4;
    if (need > wpart) wpart = need;
  }
  q.h1 = take(R1 * s.c1 * 4); q.h2 = take(R2 * s.c2 * 4);
  q.g3 = take(R2 * 8 * s.c * 4); q.dh2 = take(R2 * s.c2 * 4); q.dh1 = take(R1 * s.c1 * 4);
  q.wpart = take(wpart);
  const size_t ln1 = (size_t)cdiv(R1, kDtLnRows) * s.c1, ln2 = (size_t)cdiv(R2, kDtLnRows) * s.c2;
  q.lnpart = take(3 * (ln1 > ln2 ? ln1 : ln2) * 4);
  q.colpart = take((size_t)cdiv(R2, kDtColRows) * 8 * s.c * 4);
  q.nplchunk = cdiv(s.V(), kDtPlaneChunk);
  q.plpart = take((size_t)s.n * s.c * q.nplchunk * 2 * 4);
  q.bstat = take((size_t)s.n * s.c * 8);
  q.bytes = o;
  *out = q;
  return true;
}

__device__ __forceinline__ float dt_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// W [pairs = cin cout][8] -> bp[ci][k cout + co] and bt[k cout + co][ci] (either may be null).  grid ceil(pairs / 256), block 256
__global__ __launch_bounds__(256) void dt_pack_kernel(const float* __restrict__ w, int cin, int cout, float* __restrict__ bp, float* __restrict__ bt) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)cin * cout) return;
  const int ci = (int)(i / cout), co = (int)(i % cout);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float v = w[i * 8 + k];
    if (bp) bp[(long long)ci * 8 * cout + k * cout + co] = v;
    if (bt) bt[((long long)k * cout + co) * cin + ci] = v;
  }
}

struct DtGemm {
  const float* a; long long lda;      // !TA: A[m][k] = a[m lda + k];  TA: A[m][k] = a[k lda + m]
  const float* b; long long ldb;      // B[k][n] = b[k ldb + n]
  int M, N;
  long long K, kchunk;                // workgroup z sums k in [z kchunk, min(K, (z + 1) kchunk)) into out + z M N
  const float* bias; int cout;        // bias[n % cout], or null
  float* out; long long ldc;
  int T, gh, gw, C;                   // DT_EPI_PLANAR: tokens per view, grid, output channels
};

// grid (ceil(M / 64), ceil(N / 64), splits), block 256.  Wave w owns the 32 x 32 quadrant (w >> 1, w & 1) as 2 x 2 MFMA tiles; lane l feeds
// A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15] and holds D[4 (l >> 4) + v][l & 15], v < 4.  Everything outside M, N, K is zero-filled
// on the way into LDS and masked on the way out.
template <bool TA, int EPI>
__global__ __launch_bounds__(256) void dt_gemm_kernel(DtGemm p) {
  __shared__ float As[kDtTK][kDtLD];
  __shared__ float Bs[kDtTK][kDtLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * kDtTM, n0 = blockIdx.y * kDtTN;
  const long long kb = (long long)blockIdx.z * p.kchunk;
  const long long ke = kb + p.kchunk < p.K ? kb + p.kchunk : p.K;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, lr = lane & 15, lq = lane >> 4;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long k0 = kb; k0 < ke; k0 += kDtTK) {
    if (TA) {
      const int m = tid & 63;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = (tid >> 6) + 4 * i;
        As[k][m] = (k0 + k < ke && m0 + m < p.M) ? p.a[(k0 + k) * p.lda + m0 + m] : 0.f;
      }
    } else {
      const int k = tid & 15;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = (tid >> 4) + 16 * i;
        As[k][m] = (k0 + k < ke && m0 + m < p.M) ? p.a[(long long)(m0 + m) * p.lda + k0 + k] : 0.f;
      }
    }
    {
      const int n = tid & 63;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = (tid >> 6) + 4 * i;
        Bs[k][n] = (k0 + k < ke && n0 + n < p.N) ? p.b[(k0 + k) * p.ldb + n0 + n] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kDtTK; kk += 4) {
      const float a0 = As[kk + lq][wm + lr], a1 = As[kk + lq][wm + 16 + lr];
      const float b0 = Bs[kk + lq][wn + lr], b1 = Bs[kk + lq][wn + 16 + lr];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  float* out = p.out + (EPI == DT_EPI_ROWS ? (long long)blockIdx.z * p.M * p.N : 0);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = m0 + wm + i * 16 + 4 * lq + v;
      if (row >= p.M) continue;
      long long base;
      int bz = 0, by = 0, bx = 0;
      if (EPI == DT_EPI_PLANAR) {
        // row = ((n T + t) 8 + k1) 8 + k2 -> the corner of its 2 x 2 x 2 block of voxels
        const int k2 = row & 7, k1 = (row >> 3) & 7, nt = row >> 6, n = nt / p.T, t = nt % p.T;
        const int tz = t / (p.gh * p.gw), ty = t / p.gw % p.gh, tx = t % p.gw;
        bz = 8 * tz + 4 * (k1 >> 2) + 2 * (k2 >> 2);
        by = 8 * ty + 4 * ((k1 >> 1) & 1) + 2 * ((k2 >> 1) & 1);
        bx = 8 * tx + 4 * (k1 & 1) + 2 * (k2 & 1);
        base = (long long)n * p.C;
      } else {
        base = (long long)row * p.ldc;
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn + j * 16 + lr;
        if (col >= p.N) continue;
        const float val = acc[i][j][v] + (p.bias ? p.bias[col % p.cout] : 0.f);
        if (EPI == DT_EPI_PLANAR) {
          const int k3 = col / p.C, c = col % p.C;
          const long long H = 8LL * p.gh, W = 8LL * p.gw, D = 8LL * (p.T / (p.gh * p.gw));
          out[(((base + c) * D + bz + (k3 >> 2)) * H + by + ((k3 >> 1) & 1)) * W + bx + (k3 & 1)] = val;
        } else {
          out[base + col] = val;
        }
      }
    }
}

__device__ __forceinline__ float dt_gelu(float y) { return 0.5f * y * (1.f + erff(y * 0.70710678118654752f)); }
__device__ __forceinline__ float dt_gelu_grad(float y) {
  return 0.5f * (1.f + erff(y * 0.70710678118654752f)) + y * 0.39894228040143268f * expf(-0.5f * y * y);
}

// h[r] = GELU(w (a[r] - mean) rstd + b) over the C <= 384 channels of row r.  st_in: the row's saved {mean, rstd}; null: computed (two
// passes over the registers) and stored to st_out.  grid ceil(R / 4), block 256: one wave per row
__global__ __launch_bounds__(256) void dt_ln_kernel(const float* __restrict__ a, long long R, int C, const float* __restrict__ w,
                                                    const float* __restrict__ b, float eps, const float* __restrict__ st_in,
                                                    float* __restrict__ st_out, float* __restrict__ h) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;                                        // (wave-uniform; no barrier in this kernel)
  const float* row = a + r * C;
  float x[kDtLnMax];
#pragma unroll
  for (int i = 0; i < kDtLnMax; ++i) x[i] = lane + 64 * i < C ? row[lane + 64 * i] : 0.f;
  float mean, rstd;
  if (st_in) {
    mean = st_in[2 * r]; rstd = st_in[2 * r + 1];
  } else {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kDtLnMax; ++i) s += x[i];
    mean = dt_wave_sum(s) / (float)C;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < kDtLnMax; ++i)
      if (lane + 64 * i < C) { const float d = x[i] - mean; v = fmaf(d, d, v); }
    rstd = 1.f / sqrtf(dt_wave_sum(v) / (float)C + eps);
    if (lane == 0) { st_out[2 * r] = mean; st_out[2 * r + 1] = rstd; }
  }
#pragma unroll
  for (int i = 0; i < kDtLnMax; ++i) {
    const int c = lane + 64 * i;
    if (c < C) h[r * C + c] = dt_gelu(fmaf((x[i] - mean) * rstd, w[c], b[c]));
  }
}

// The adjoint of dt_ln for the rows [128 wg, 128 wg + 128): g (the gradient of h) becomes da IN PLACE, and the workgroup's sums of
// dy x^ (dgamma), dy (dbeta) and da (the conv bias in front) go to part[which][wg][C].  Wave w walks rows w, w + 4, ...; the four waves'
// sums are added in wave order.  grid ceil(R / 128), block 256
__global__ __launch_bounds__(256) void dt_ln_bwd_kernel(const float* __restrict__ a, const float* __restrict__ st, long long R, int C,
                                                        const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ g,
                                                        float* __restrict__ part) {
  __shared__ float ps[4][3][64 * kDtLnMax];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * kDtLnRows;
  float wv[kDtLnMax], bv[kDtLnMax], sg[kDtLnMax], sb[kDtLnMax], sa[kDtLnMax];
#pragma unroll
  for (int i = 0; i < kDtLnMax; ++i) {
    const int c = lane + 64 * i;
    wv[i] = c < C ? w[c] : 0.f; bv[i] = c < C ? b[c] : 0.f;
    sg[i] = sb[i] = sa[i] = 0.f;
  }
  for (int j = wave; j < kDtLnRows; j += 4) {
    const long long r = r0 + j;
    if (r >= R) break;                                       // (wave-uniform)
    const float mean = st[2 * r], rstd = st[2 * r + 1];
    float xh[kDtLnMax], d[kDtLnMax];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < kDtLnMax; ++i) {
      const int c = lane + 64 * i;
      xh[i] = 0.f; d[i] = 0.f;
      if (c < C) {
        xh[i] = (a[r * C + c] - mean) * rstd;
        const float dy = g[r * C + c] * dt_gelu_grad(fmaf(xh[i], wv[i], bv[i]));
        sg[i] = fmaf(dy, xh[i], sg[i]); sb[i] += dy;
        d[i] = dy * wv[i];
        s1 += d[i]; s2 = fmaf(d[i], xh[i], s2);
      }
    }
    const float m1 = dt_wave_sum(s1) / (float)C, m2 = dt_wave_sum(s2) / (float)C;
#pragma unroll
    for (int i = 0; i < kDtLnMax; ++i) {
      const int c = lane + 64 * i;
      if (c < C) {
        const float da = rstd * (d[i] - m1 - xh[i] * m2);
        g[r * C + c] = da;
        sa[i] += da;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kDtLnMax; ++i) {
    ps[wave][0][lane + 64 * i] = sg[i]; ps[wave][1][lane + 64 * i] = sb[i]; ps[wave][2][lane + 64 * i] = sa[i];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 3 * C; idx += 256) {
    const int which = idx / C, c = idx % C;
    part[((long long)which * gridDim.x + blockIdx.x) * C + c] = ((ps[0][which][c] + ps[1][which][c]) + ps[2][which][c]) + ps[3][which][c];
  }
}

// part[wg][c] = sum of src[r][c] over the rows [256 wg, 256 wg + 256), r ascending.  grid ceil(R / 256), block 256 (C <= 1024)
__global__ __launch_bounds__(256) void dt_colpart_kernel(const float* __restrict__ src, long long R, int C, float* __restrict__ part) {
  const long long r0 = (long long)blockIdx.x * kDtColRows;
  const long long r1 = r0 + kDtColRows < R ? r0 + kDtColRows : R;
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (long long r0b = r0; r0b < r1; r0b += 16) {          // 16 rows first, then one addition to the running sum
      float t = 0.f;
      for (long long r = r0b; r < r0b + 16 && r < r1; ++r) t += src[r * C + c];
      s += t;
    }
    part[(long long)blockIdx.x * C + c] = s;
  }
}

// dst[c] = sum over k < fold (ascending) of the sum over the nb rows of src[.][k C + c] (ld = fold C).  Wave w adds rows w, w + 4, ... (16
// at a time), the four sums are added in wave order.  grid ceil(C / 64), block 256
__global__ __launch_bounds__(256) void dt_colreduce_kernel(const float* __restrict__ src, int nb, int C, int fold, float* __restrict__ dst) {
  __shared__ float ps[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
  const long long ld = (long long)fold * C;
  float total = 0.f;
  for (int k = 0; k < fold; ++k) {
    float s = 0.f;
    if (c < C)
      for (int r0 = wave; r0 < nb; r0 += 64) {
        float t = 0.f;
        for (int r = r0; r < r0 + 64 && r < nb; r += 4) t += src[r * ld + (long long)k * C + c];
        s += t;
      }
    ps[wave][lane] = s;
    __syncthreads();
    total += ((ps[0][lane] + ps[1][lane]) + ps[2][lane]) + ps[3][lane];
    __syncthreads();
  }
  if (wave == 0 && c < C) dst[c] = total;
}

// dw[ci][co][k] = sum over the splits s (ascending, 16 at a time) of part[s][ci][k cout + co].  grid ceil(cin cout 8 / 256), block 256
__global__ __launch_bounds__(256) void dt_wreduce_kernel(const float* __restrict__ part, int splits, int cin, int cout, float* __restrict__ dw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, total = (long long)cin * cout * 8;
  if (i >= total) return;
  const int k = (int)(i & 7), co = (int)((i >> 3) % cout), ci = (int)((i >> 3) / cout);
  const float* src = part + (long long)ci * 8 * cout + k * cout + co;
  float s = 0.f;
  for (int s0 = 0; s0 < splits; s0 += 16) {
    float t = 0.f;
    for (int j = s0; j < s0 + 16 && j < splits; ++j) t += src[(long long)j * total];
    s += t;
  }
  dw[i] = s;
}

// Per plane nc of V voxels and chunk of 8192: part[(nc nchunk + chunk) 2 + {0, 1}] =
//   MODE 0: {sum x, -};  MODE 1: {sum (x - mean)^2, -} with mean = stat[2 nc];  MODE 2: {sum x, sum x y}
// Thread sums (stride 256), the butterfly of each wave, then the four waves in order.  grid (nchunk, planes), block 256
template <int MODE>
__global__ __launch_bounds__(256) void dt_plane_partial_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ stat,
                                                               long long V, float* __restrict__ part) {
  __shared__ float ps[4][2];
  const int nc = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long b = (long long)blockIdx.x * kDtPlaneChunk, e = b + kDtPlaneChunk < V ? b + kDtPlaneChunk : V;
  const float* px = x + (long long)nc * V;
  const float* py = (MODE == 2 && y) ? y + (long long)nc * V : nullptr;
  const float mean = MODE == 1 ? stat[2 * nc] : 0.f;
  float s0 = 0.f, s1 = 0.f;
  for (long long i = b + threadIdx.x; i < e; i += 256) {
    const float v = px[i];
    if (MODE == 0) s0 += v;
    if (MODE == 1) { const float d = v - mean; s0 = fmaf(d, d, s0); }
    if (MODE == 2) { s0 += v; if (py) s1 = fmaf(v, py[i], s1); }
  }
  s0 = dt_wave_sum(s0); s1 = dt_wave_sum(s1);
  if (lane == 0) { ps[wave][0] = s0; ps[wave][1] = s1; }
  __syncthreads();
  if (threadIdx.x < 2)
    part[((long long)nc * gridDim.x + blockIdx.x) * 2 + threadIdx.x] =
        ((ps[0][threadIdx.x] + ps[1][threadIdx.x]) + ps[2][threadIdx.x]) + ps[3][threadIdx.x];
}

// The chunks of a plane added in double, ascending.  MODE 0: stat = {sum / V, 1};  1: stat[1] = 1 / sqrt(sum / V + eps);  2: stat =
// {sum0 / V, sum1 / V}.  grid ceil(planes / 256), block 256
__global__ __launch_bounds__(256) void dt_plane_final_kernel(const float* __restrict__ part, int planes, int nchunk, long long V, float eps, int mode,
                                                             float* __restrict__ stat) {
  const int nc = blockIdx.x * 256 + threadIdx.x;
  if (nc >= planes) return;
  double s0 = 0.0, s1 = 0.0;
  for (int j = 0; j < nchunk; ++j) { s0 += (double)part[((long long)nc * nchunk + j) * 2]; s1 += (double)part[((long long)nc * nchunk + j) * 2 + 1]; }
  if (mode == 0) { stat[2 * nc] = (float)(s0 / (double)V); stat[2 * nc + 1] = 1.f; }
  if (mode == 1) stat[2 * nc + 1] = (float)(1.0 / sqrt(s0 / (double)V + (double)eps));
  if (mode == 2) { stat[2 * nc] = (float)(s0 / (double)V); stat[2 * nc + 1] = (float)(s1 / (double)V); }
}

// x = (x - mean) rstd in place, {mean, rstd} = stat[2 nc ..].  grid (ceil(V / 1024), planes), block 256
__global__ __launch_bounds__(256) void dt_plane_apply_kernel(float* __restrict__ x, const float* __restrict__ stat, long long V) {
  const int nc = blockIdx.y;
  const float mean = stat[2 * nc], rstd = stat[2 * nc + 1];
  float* px = x + (long long)nc * V;
  const long long b = (long long)blockIdx.x * 1024;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long j = b + threadIdx.x + 256 * i;
    if (j < V) px[j] = (px[j] - mean) * rstd;
  }
}

// g3[r2][k3 C + c] = the gradient of the decoder's raw output at voxel (n, c, z, y, x), from planar dy through the output norm's adjoint:
//   none: dy;   demean: dy - m1;   instance: rstd (dy - m1 - y m2)   with {m1, m2} = bstat[2 nc ..] (the plane's means of dy and dy y),
//   rstd = ostat[2 nc + 1] and y the forward's normalised output.  grid ceil(total / 256), block 256
__global__ __launch_bounds__(256) void dt_gather_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ ostat,
                                                        const float* __restrict__ bstat, int mode, long long total, int C, int gd, int gh, int gw,
                                                        float* __restrict__ g3) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int D = 8 * gd, H = 8 * gh, W = 8 * gw;
  const int x = (int)(idx % W), yy = (int)(idx / W % H), z = (int)(idx / ((long long)W * H) % D), nc = (int)(idx / ((long long)W * H * D));
  const int c = nc % C, n = nc / C;
  float v = dy[idx];
  if (mode == DT_NORM_DEMEAN) v -= bstat[2 * nc];
  if (mode == DT_NORM_INSTANCE) v = ostat[2 * nc + 1] * (v - bstat[2 * nc] - y[idx] * bstat[2 * nc + 1]);
  const long long t = ((long long)(z >> 3) * gh + (yy >> 3)) * gw + (x >> 3);
  const int k1 = (((z >> 2) & 1) << 2) | (((yy >> 2) & 1) << 1) | ((x >> 2) & 1);
  const int k2 = (((z >> 1) & 1) << 2) | (((yy >> 1) & 1) << 1) | ((x >> 1) & 1);
  const int k3 = ((z & 1) << 2) | ((yy & 1) << 1) | (x & 1);
  const long long r2 = (((long long)n * gd * gh * gw + t) * 8 + k1) * 8 + k2;
  g3[r2 * 8 * C + k3 * C + c] = v;
}

struct DtCall {
  DtShape s;
  DtPlan q;
  const float* tokens;
  const float* prm[kDtParams];
  float ln_eps, out_eps;
  int out_norm;
  char *sv, *sc;
  hipStream_t st;
  template <typename T> T* saved(size_t off) const { return (T*)(sv + off); }
  template <typename T> T* at(size_t off) const { return (T*)(sc + off); }
};

#define DT_TRY(expr)                          \
  do {                                        \
    hipError_t e_ = (expr);                   \
    if (e_ != hipSuccess) return e_;          \
  } while (0)
#define DT_LAUNCHED() DT_TRY(hipGetLastError())

// out [M][ldc] = A [M][K] B [K][N] + bias[n % cout]
hipError_t dt_product(const DtCall& c, int epi, const float* a, long long M, int K, const float* b, int N, const float* bias, int cout, float* out) {
  DtGemm p{};
  p.a = a; p.lda = K; p.b = b; p.ldb = N; p.M = (int)M; p.N = N; p.K = K; p.kchunk = K; p.bias = bias; p.cout = cout; p.out = out; p.ldc = N;
  p.T = (int)c.s.T(); p.gh = c.s.gh; p.gw = c.s.gw; p.C = c.s.c;
  const dim3 grid(cdiv(M, kDtTM), cdiv(N, kDtTN), 1);
  if (epi == DT_EPI_PLANAR)
    hipLaunchKernelGGL((dt_gemm_kernel<false, DT_EPI_PLANAR>), grid, dim3(256), 0, c.st, p);
  else
    hipLaunchKernelGGL((dt_gemm_kernel<false, DT_EPI_ROWS>), grid, dim3(256), 0, c.st, p);
  return hipGetLastError();
}

// dw [cin][cout][8] = sum over the R rows of x[r][ci] g[r][k cout + co]: partials per chunk of rows, then their sum
hipError_t dt_wgrad(const DtCall& c, int stage, const float* x, const float* g, long long R, int cin, int cout, float* dw) {
  DtGemm p{};
  float* part = c.at<float>(c.q.wpart);
  p.a = x; p.lda = cin; p.b = g; p.ldb = 8 * cout; p.M = cin; p.N = 8 * cout; p.K = R; p.kchunk = c.q.wchunk[stage]; p.out = part; p.ldc = 8 * cout;
  hipLaunchKernelGGL((dt_gemm_kernel<true, DT_EPI_ROWS>), dim3(cdiv(cin, kDtTM), cdiv(8 * cout, kDtTN), c.q.wsplit[stage]), dim3(256), 0, c.st, p);
  DT_LAUNCHED();
  hipLaunchKernelGGL(dt_wreduce_kernel, dim3(cdiv((long long)cin * cout * 8, 256)), dim3(256), 0, c.st, part, c.q.wsplit[stage], cin, cout, dw);
  return hipGetLastError();
}

hipError_t dt_pack(const DtCall& c, bool fwd) {
  const int cin[3] = {c.s.e, c.s.c1, c.s.c2}, cout[3] = {c.s.c1, c.s.c2, c.s.c}, wi[3] = {W1, W2, W3};
  for (int i = 0; i < 3; ++i) {
    hipLaunchKernelGGL(dt_pack_kernel, dim3(cdiv((long long)cin[i] * cout[i], 256)), dim3(256), 0, c.st, c.prm[wi[i]], cin[i], cout[i],
                       fwd ? c.at<float>(c.q.bp[i]) : nullptr, fwd ? nullptr : c.at<float>(c.q.bt[i]));
    DT_LAUNCHED();
  }
  return hipSuccess;
}

hipError_t dt_ln(const DtCall& c, const float* a, long long R, int C, const float* w, const float* b, const float* st_in, float* st_out, float* h) {
  hipLaunchKernelGGL(dt_ln_kernel, dim3(cdiv(R, 4)), dim3(256), 0, c.st, a, R, C, w, b, c.ln_eps, st_in, st_out, h);
  return hipGetLastError();
}

// sum of the nb partial rows [fold C] -> dst[C]
hipError_t dt_colreduce(const DtCall& c, const float* part, int nb, int C, int fold, float* dst) {
  hipLaunchKernelGGL(dt_colreduce_kernel, dim3(cdiv(C, 64)), dim3(256), 0, c.st, part, nb, C, fold, dst);
  return hipGetLastError();
}

// g [R][C] -> da in place; dgamma, dbeta and the bias gradient where asked
hipError_t dt_ln_bwd(const DtCall& c, const float* a, const float* st, long long R, int C, const float* w, const float* b, float* g, float* dgamma,
                     float* dbeta, float* dbias) {
  float* part = c.at<float>(c.q.lnpart);
  const int nb = cdiv(R, kDtLnRows);
  hipLaunchKernelGGL(dt_ln_bwd_kernel, dim3(nb), dim3(256), 0, c.st, a, st, R, C, w, b, g, part);
  DT_LAUNCHED();
  float* dst[3] = {dgamma, dbeta, dbias};
  for (int i = 0; i < 3; ++i)
    if (dst[i]) DT_TRY(dt_colreduce(c, part + (size_t)i * nb * C, nb, C, 1, dst[i]));
  return hipSuccess;
}

template <int MODE>
hipError_t dt_plane_stats(const DtCall& c, const float* x, const float* y, const float* stat_in, float* stat_out) {
  const int planes = c.s.n * c.s.c;
  float* part = c.at<float>(c.q.plpart);
  hipLaunchKernelGGL((dt_plane_partial_kernel<MODE>), dim3(c.q.nplchunk, planes), dim3(256), 0, c.st, x, y, stat_in, c.s.V(), part);
  DT_LAUNCHED();
  hipLaunchKernelGGL(dt_plane_final_kernel, dim3(cdiv(planes, 256)), dim3(256), 0, c.st, part, planes, c.q.nplchunk, c.s.V(), c.out_eps, MODE, stat_out);
  return hipGetLastError();
}

hipError_t dt_forward(const DtCall& c, float* out) {
  const DtShape& s = c.s;
  const DtPlan& q = c.q;
  DT_TRY(dt_pack(c, true));
  float *a1 = c.saved<float>(q.a1), *a2 = c.saved<float>(q.a2), *st1 = c.saved<float>(q.st1), *st2 = c.saved<float>(q.st2);
  float *h1 = c.at<float>(q.h1), *h2 = c.at<float>(q.h2);
  DT_TRY(dt_product(c, DT_EPI_ROWS, c.tokens, s.R0(), s.e, c.at<float>(q.bp[0]), 8 * s.c1, c.prm[B1], s.c1, a1));
  DT_TRY(dt_ln(c, a1, s.R1(), s.c1, c.prm[LW1], c.prm[LB1], nullptr, st1, h1));
  DT_TRY(dt_product(c, DT_EPI_ROWS, h1, s.R1(), s.c1, c.at<float>(q.bp[1]), 8 * s.c2, c.prm[B2], s.c2, a2));
  DT_TRY(dt_ln(c, a2, s.R2(), s.c2, c.prm[LW2], c.prm[LB2], nullptr, st2, h2));
  DT_TRY(dt_product(c, DT_EPI_PLANAR, h2, s.R2(), s.c2, c.at<float>(q.bp[2]), 8 * s.c, c.prm[B3], s.c, out));
  if (c.out_norm != DT_NORM_NONE) {
    float* ostat = c.saved<float>(q.ostat);
    DT_TRY(dt_plane_stats<0>(c, out, nullptr, nullptr, ostat));
    if (c.out_norm == DT_NORM_INSTANCE) DT_TRY(dt_plane_stats<1>(c, out, nullptr, ostat, ostat));
    hipLaunchKernelGGL(dt_plane_apply_kernel, dim3(cdiv(s.V(), 1024), s.n * s.c), dim3(256), 0, c.st, out, ostat, s.V());
    DT_LAUNCHED();
  }
  return hipSuccess;
}

hipError_t dt_backward(const DtCall& c, const float* dout, const float* y, float* dtokens, float* const* g) {
  const DtShape& s = c.s;
  const DtPlan& q = c.q;
  DT_TRY(dt_pack(c, false));
  const float *a1 = c.saved<float>(q.a1), *a2 = c.saved<float>(q.a2), *st1 = c.saved<float>(q.st1), *st2 = c.saved<float>(q.st2);
  float *h1 = c.at<float>(q.h1), *h2 = c.at<float>(q.h2), *g3 = c.at<float>(q.g3), *dh2 = c.at<float>(q.dh2), *dh1 = c.at<float>(q.dh1);
  if (g[W2]) DT_TRY(dt_ln(c, a1, s.R1(), s.c1, c.prm[LW1], c.prm[LB1], st1, nullptr, h1));
  if (g[W3]) DT_TRY(dt_ln(c, a2, s.R2(), s.c2, c.prm[LW2], c.prm[LB2], st2, nullptr, h2));
  // output norm adjoint + gather into nested rows
  float* bstat = c.at<float>(q.bstat);
  if (c.out_norm == DT_NORM_DEMEAN) DT_TRY(dt_plane_stats<2>(c, dout, nullptr, nullptr, bstat));
  if (c.out_norm == DT_NORM_INSTANCE) DT_TRY(dt_plane_stats<2>(c, dout, y, nullptr, bstat));
  const long long total = (long long)s.n * s.c * s.V();
  hipLaunchKernelGGL(dt_gather_kernel, dim3(cdiv(total, 256)), dim3(256), 0, c.st, dout, y, c.saved<float>(q.ostat), bstat, c.out_norm, total, s.c,
                     s.gd, s.gh, s.gw, g3);
  DT_LAUNCHED();
  // stage 3
  if (g[B3]) {
    const int nb = cdiv(s.R2(), kDtColRows);
    hipLaunchKernelGGL(dt_colpart_kernel, dim3(nb), dim3(256), 0, c.st, g3, s.R2(), 8 * s.c, c.at<float>(q.colpart));
    DT_LAUNCHED();
    DT_TRY(dt_colreduce(c, c.at<float>(q.colpart), nb, s.c, 8, g[B3]));
  }
  if (g[W3]) DT_TRY(dt_wgrad(c, 2, h2, g3, s.R2(), s.c2, s.c, g[W3]));
  DT_TRY(dt_product(c, DT_EPI_ROWS, g3, s.R2(), 8 * s.c, c.at<float>(q.bt[2]), s.c2, nullptr, 1, dh2));
  // stage 2: da2 [R2][c2] read as [R1][8 c2] is g2
  DT_TRY(dt_ln_bwd(c, a2, st2, s.R2(), s.c2, c.prm[LW2], c.prm[LB2], dh2, g[LW2], g[LB2], g[B2]));
  if (g[W2]) DT_TRY(dt_wgrad(c, 1, h1, dh2, s.R1(), s.c1, s.c2, g[W2]));
  DT_TRY(dt_product(c, DT_EPI_ROWS, dh2, s.R1(), 8 * s.c2, c.at<float>(q.bt[1]), s.c1, nullptr, 1, dh1));
  // stage 1: da1 [R1][c1] read as [R0][8 c1] is g1
  DT_TRY(dt_ln_bwd(c, a1, st1, s.R1(), s.c1, c.prm[LW1], c.prm[LB1], dh1, g[LW1], g[LB1], g[B1]));
  if (g[W1]) DT_TRY(dt_wgrad(c, 0, c.tokens, dh1, s.R0(), s.e, s.c1, g[W1]));
  if (dtokens) DT_TRY(dt_product(c, DT_EPI_ROWS, dh1, s.R0(), 8 * s.c1, c.at<float>(q.bt[0]), s.e, nullptr, 1, dtokens));
  return hipSuccess;
}

// the checks both entries share: AMX_OK and a filled call, or the refusal -- before any launch
int dt_prepare(const char* what, const float* d_tokens, const void* const* params, int n, int gd, int gh, int gw, int e, int c1, int c2, int c,
               float ln_eps, int out_norm, float out_eps, const void* d_saved, size_t saved_bytes, void* d_scratch, size_t scratch_bytes, void* stream,
               DtCall* call) {
  if (!d_tokens || !params) return fail(AMX_ERR_INVALID, "%s: null argument", what);
  DtCall k{};
  k.s = DtShape{n, gd, gh, gw, e, c1, c2, c};
  if (!dt_plan(k.s, &k.q))
    return fail(AMX_ERR_SHAPE,
                "%s: views %d, token grid (%d, %d, %d), widths %d / %d / %d / %d are outside the envelope (patch 8; widths multiples of 4 up to "
                "%d / %d / %d, 1 .. %d output channels, views x channels up to 65535, every tensor below 2^31 elements)",
                what, n, gd, gh, gw, e, c1, c2, c, kDtMaxE, kDtMaxC1, kDtMaxC2, kDtMaxC);
  if (out_norm < 0 || out_norm > 2) return fail(AMX_ERR_INVALID, "%s: out_norm is 0 (none), 1 (demean) or 2 (instance), got %d", what, out_norm);
  for (int i = 0; i < kDtParams; ++i) k.prm[i] = (const float*)params[i];
  const int must[] = {W1, LW1, LB1, W2, LW2, LB2, W3};
  for (int i : must)
    if (!k.prm[i]) return fail(AMX_ERR_INVALID, "%s: params[%d] is null (only the conv biases may be)", what, i);
  if (!d_saved || saved_bytes < k.q.saved_bytes || ((uintptr_t)d_saved & 15))
    return fail(AMX_ERR_WORKSPACE, "%s: saved state needs %zu bytes, 16-byte aligned", what, k.q.saved_bytes);
  if (!d_scratch || scratch_bytes < k.q.bytes || ((uintptr_t)d_scratch & 15))
    return fail(AMX_ERR_WORKSPACE, "%s: scratch needs %zu bytes, 16-byte aligned", what, k.q.bytes);
  k.tokens = d_tokens; k.ln_eps = ln_eps; k.out_eps = out_eps; k.out_norm = out_norm;
  k.sv = (char*)d_saved; k.sc = (char*)d_scratch; k.st = (hipStream_t)stream;
  *call = k;
  return AMX_OK;
}

}  // namespace

}  // namespace amx

extern "C" {

size_t amx_vit_decoder_train_saved_bytes(int n, int gd, int gh, int gw, int e, int c1, int c2, int c) {
  amx::DtPlan q;
  return amx::dt_plan(amx::DtShape{n, gd, gh, gw, e, c1, c2, c}, &q) ? q.saved_bytes : 0;
}

size_t amx_vit_decoder_train_scratch_bytes(int n, int gd, int gh, int gw, int e, int c1, int c2, int c) {
  amx::DtPlan q;
  return amx::dt_plan(amx::DtShape{n, gd, gh, gw, e, c1, c2, c}, &q) ? q.bytes : 0;
}

int amx_vit_decoder_train_forward(const float* d_tokens, const void* const* params, int n, int gd, int gh, int gw, int e, int c1, int c2, int c,
                                  float ln_eps, int out_norm, float out_eps, float* d_out, void* d_saved, size_t saved_bytes, void* d_scratch,
                                  size_t scratch_bytes, void* stream) {
  amx::DtCall call;
  if (int rc = amx::dt_prepare("decoder train forward", d_tokens, params, n, gd, gh, gw, e, c1, c2, c, ln_eps, out_norm, out_eps, d_saved, saved_bytes,
                               d_scratch, scratch_bytes, stream, &call))
    return rc;
  if (!d_out) return amx::fail(AMX_ERR_INVALID, "decoder train forward: null d_out");
  AMX_HIP(amx::dt_forward(call, d_out));
  return AMX_OK;
}

int amx_vit_decoder_backward(const float* d_dout, const float* d_out, const float* d_tokens, const void* const* params, const void* d_saved,
                             size_t saved_bytes, int n, int gd, int gh, int gw, int e, int c1, int c2, int c, float ln_eps, int out_norm,
                             float out_eps, float* d_dtokens, void* const* grads, void* d_scratch, size_t scratch_bytes, void* stream) {
  amx::DtCall call;
  if (int rc = amx::dt_prepare("decoder backward", d_tokens, params, n, gd, gh, gw, e, c1, c2, c, ln_eps, out_norm, out_eps, d_saved, saved_bytes,
                               d_scratch, scratch_bytes, stream, &call))
    return rc;
  if (!d_dout || !grads) return amx::fail(AMX_ERR_INVALID, "decoder backward: null argument");
  if (out_norm == amx::DT_NORM_INSTANCE && !d_out) return amx::fail(AMX_ERR_INVALID, "decoder backward: the instance norm's adjoint reads d_out");
  float* g[amx::kDtParams];
  for (int i = 0; i < amx::kDtParams; ++i) g[i] = (float*)grads[i];
  AMX_HIP(amx::dt_backward(call, d_dout, d_out, d_dtokens, g));
  return AMX_OK;
}

}  // extern "C"
