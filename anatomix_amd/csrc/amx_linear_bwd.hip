// anatomix_amd -- the EVA blocks' nn.Linear layers under autograd: y = x W^T + b for fp32 x [M][K], W [N][K], and the three gradients
//   dx = dy W          dW[n][k] = sum_m dy[m][n] x[m][k]          db[n] = sum_m dy[m][n]
// on the f16 matrix pipe (v_mfma_f32_16x16x32_f16, fp32 accumulation).  Exactly three roundings, each operand once:
//   x^ = f16(x)      W^ = f16(W)      dy^ = f16(dy 2^-e)          (f16 subnormals kept)
// with ONE exponent e per call, 2^e <= max |dy| / 8 < 2^(e+1), found on the device (no host read-back; the attention backward's
// attn_delta / attn_dprep are the model); the gradients are multiplied by 2^e where they are stored.  An all-zero dy takes e = 0 and
// gives exact zeros.  The bias gradient is the fp32 column sum of the UNROUNDED dy.
//
// Passes:
//   forward    pack_gemm (mode 0) W -> W^ fragments; lin_image<rows> x -> x^ token rows [M][ceil32(K)]; launch_gemm EPI_F32 (+ bias).
//   backward   lin_dy_stats      max |dy| and the column sums of dy per block of rows (fp32, unrounded)
//              lin_dy_fix        the exponent -> device cell {2^-e, 2^e}; the column partials added in one fixed order -> db
//              lin_image         dy -> dy^ rows (dgrad) and dy^ / x^ COL images (wgrad)
//              dgrad             lin_pack_t W -> (W^)^T fragments; launch_gemm EPI_F32_SCALED: dx = (dy^ W^) 2^e
//              lin_wgrad         the token is the reduction index, so BOTH MFMA operands need eight consecutive tokens of one feature
//                                per lane.  The COL images are written in fragment order [feature tile][token step of 32][lane][8 halves]
//                                (lane (i, g): feature 16 tile + i, tokens 32 step + 8 g .. + 7; zeros behind the last feature / token),
//                                so an operand fragment is one coalesced 1 KiB load and the kernel needs no LDS and no transposing
//                                read.  A workgroup owns 128 x 128 (k, n) features (4 waves x 4 x 4 tiles) and one contiguous chunk of
//                                token steps; it stores fp32 partials [chunk][N][K] (a lane owns 4 consecutive k of one n: 16 bytes).
//              lin_wgrad_reduce  dW = (sum over the chunks in index order) 2^e.  No atomics anywhere: bit-identical run to run.
// Nothing is kept across calls: weights are packed per call into the scratch, the backward re-converts the saved fp32 x.
#include <limits.h>

#include "amx_device.h"
#include "amx_gemm.h"
#include "amx_launch.h"

namespace amx {

namespace {

constexpr int kLinGradExp = 3;          // max |dy^| lies in [2^3, 2^4)
constexpr int kLinStatRows = 64;        // rows per block of lin_dy_stats (more when M / 64 exceeds kLinStatMax blocks)
constexpr int kLinStatMax = 2048;
constexpr int kLinAT = 4, kLinBT = 4;   // tiles per wave of lin_wgrad along k / n; a workgroup is 2 x 2 waves
constexpr int kLinMinSteps = 16;        // token steps per chunk, at least
constexpr int kLinWantWg = 512;         // workgroups a wgrad launch aims for (2 per CU)

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct LinPlan {
  int ldk, ldn, KT, NT, KS, NS, MS;     // padded row lengths (halves); 16-feature tiles; 32-column steps of K / N; 32-token steps
  int nstat, stat_rows;                 // lin_dy_stats: blocks, rows per block
  int kblocks, nblocks, spc, chunks;    // lin_wgrad: grid, token steps per chunk
  size_t cell, amax, colpart, dyrows, dycol, xcol, wt, part;   // backward offsets
  size_t wpack, xrows, biaspad;         // forward offsets
  size_t bytes;
};

bool linear_plan(long long M, int K, int N, LinPlan* out) {
  if (M < 1 || K < 4 || N < 4 || (K & 3) || (N & 3) || K > (1 << 20) || N > (1 << 20)) return false;      // (grid extents)
  if (M > INT_MAX || M * (long long)(K > N ? K : N) > INT_MAX) return false;                             // rows and indices of launch_gemm
  LinPlan p{};
  p.ldk = (K + 31) / 32 * 32; p.ldn = (N + 31) / 32 * 32;
  p.KT = (K + 15) / 16; p.NT = (N + 15) / 16; p.KS = p.ldk / 32; p.NS = p.ldn / 32; p.MS = cdiv(M, 32);
  p.nstat = cdiv(M, kLinStatRows);
  if (p.nstat > kLinStatMax) p.nstat = kLinStatMax;
  p.stat_rows = cdiv(M, p.nstat);
  p.nstat = cdiv(M, p.stat_rows);
  p.kblocks = cdiv(p.KT, 2 * kLinAT); p.nblocks = cdiv(p.NT, 2 * kLinBT);
  const int want = cdiv(kLinWantWg, (long long)p.kblocks * p.nblocks);
  p.spc = cdiv(p.MS, want);
  if (p.spc < kLinMinSteps) p.spc = kLinMinSteps;
  if (p.spc > p.MS) p.spc = p.MS;
  p.chunks = cdiv(p.MS, p.spc);
  size_t o = 0;
  p.cell = o; o += 256;
  p.amax = o; o += up256((size_t)p.nstat * cdiv(N, 256) * 4);
  p.colpart = o; o += up256((size_t)p.nstat * N * 4);
  p.dyrows = o; o += up256((size_t)M * p.ldn * 2);
  p.dycol = o; o += (size_t)p.NT * p.MS * 1024;
  p.xcol = o; o += (size_t)p.KT * p.MS * 1024;
  p.wt = o; o += (size_t)p.KT * p.NS * 1024;
  p.part = o; o += up256((size_t)p.chunks * N * K * 4);
  const size_t bwd = o;
  o = 0;
  p.wpack = o; o += (size_t)p.NT * p.KS * 1024;
  p.xrows = o; o += up256((size_t)M * p.ldk * 2);
  p.biaspad = o; o += up256((size_t)p.NT * 16 * 4);
  p.bytes = bwd > o ? bwd : o;
  *out = p;
  return true;
}

// fp32 [M][C] (times the power of two in cell[0], or 1) -> f16: token rows [M][ld] with zero padding columns (ROWS) and / or the COL
// image [CT][MS][64][8] (COLS).  grid (MS, ceil(C / 64)), block 256: 32 tokens x 64 columns, 8 columns per thread.
template <bool ROWS, bool COLS>
__global__ __launch_bounds__(256) void lin_image_kernel(const float* __restrict__ src, long long M, int C, int ld, int CT, int MS,
                                                        const float* __restrict__ cell, f16* __restrict__ rows, f16* __restrict__ cols) {
  __shared__ __attribute__((aligned(16))) unsigned short tile[32][72];      // [token][column], 8 halves of padding per row
  const int tid = threadIdx.x, ms = blockIdx.x, c0 = blockIdx.y * 64;
  const float s = cell ? cell[0] : 1.f;
  const int r = tid >> 3, cc = c0 + (tid & 7) * 8;
  const long long m = (long long)ms * 32 + r;
  unsigned short h[8];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = cc + 4 * q;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m < M && c < C) v = *(const float4*)(src + m * C + c);        // C % 4 == 0: a quad is inside or outside
    h[4 * q] = to_bits<f16>(v.x * s); h[4 * q + 1] = to_bits<f16>(v.y * s);
    h[4 * q + 2] = to_bits<f16>(v.z * s); h[4 * q + 3] = to_bits<f16>(v.w * s);
  }
  const uint4 pk = make_uint4(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16), h[6] | ((unsigned)h[7] << 16));
  if (ROWS && m < M && cc < ld) *(uint4*)(rows + m * ld + cc) = pk;   // ld % 32 == 0: the 8 columns are inside or outside
  if (COLS) {
    *(uint4*)&tile[r][(tid & 7) * 8] = pk;
    __syncthreads();
    const int tt = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4, ct = blockIdx.y * 4 + tt;
    unsigned short e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = tile[8 * g + j][tt * 16 + i];
    if (ct < CT)
      *(uint4*)(cols + (((long long)ct * MS + ms) * 64 + lane) * 8) =
          make_uint4(e[0] | ((unsigned)e[1] << 16), e[2] | ((unsigned)e[3] << 16), e[4] | ((unsigned)e[5] << 16), e[6] | ((unsigned)e[7] << 16));
  }
}

// (W^)^T as the packed operand of launch_gemm: fragment [k tile][n step][lane (i, g)][e] = f16(W[32 step + 8 g + e][16 tile + i])
__global__ void lin_pack_t_kernel(const float* __restrict__ w, int N, int K, int KT, int NS, f16* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)KT * NS * 64) return;
  const int lane = idx & 63, ns = (idx >> 6) % NS, kt = (idx >> 6) / NS;
  const int k = kt * 16 + (lane & 15), n0 = ns * 32 + (lane >> 4) * 8;
  unsigned short h[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) h[e] = to_bits<f16>(k < K && n0 + e < N ? w[(long long)(n0 + e) * K + k] : 0.f);
  ((uint4*)out)[idx] = make_uint4(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16), h[6] | ((unsigned)h[7] << 16));
}

// per block of `rows` token rows and 64 column quads: amax[block] = max |dy|, colpart[row block][n] = sum of dy[.][n].  grid
// (row blocks, ceil(N / 256)), block 256: wave w adds rows w, w + 4, ... of its quad (16-byte loads), then thread (0, quad) adds the four
// waves' sums in wave order -- one fixed order.
__global__ __launch_bounds__(256) void lin_dy_stats_kernel(const float* __restrict__ dy, long long M, int N, int rows,
                                                           float* __restrict__ amax, float* __restrict__ colpart) {
  __shared__ float4 psum[4][64];
  __shared__ float wmax[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = (blockIdx.y * 64 + lane) * 4;
  const long long r0 = (long long)blockIdx.x * rows;
  const long long r1 = r0 + rows < M ? r0 + rows : M;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  float am = 0.f;
  if (c < N)                                                           // N % 4 == 0: the quad is inside or outside
    for (long long r = r0 + wave; r < r1; r += 4) {
      const float4 v = *(const float4*)(dy + r * N + c);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      am = fmaxf(fmaxf(am, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
  for (int o = 32; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 64));
  psum[wave][lane] = s;
  if (lane == 0) wmax[wave] = am;
  __syncthreads();
  if (wave == 0 && c < N) {
    float4 t = psum[0][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) { t.x += psum[w][lane].x; t.y += psum[w][lane].y; t.z += psum[w][lane].z; t.w += psum[w][lane].w; }
    *(float4*)(colpart + (long long)blockIdx.x * N + c) = t;
  }
  if (threadIdx.x == 0) amax[blockIdx.x * gridDim.y + blockIdx.y] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

// the call's power of two (workgroup 0 stores the cell) and the bias gradient in one fixed order: wave w of a workgroup adds the row
// blocks w, w + 4, ... of its 64 columns into four interleaved sums (independent loads in flight), thread (0, column) adds the waves' sums
// in wave order.  grid ceil(N / 64), block 256
__global__ __launch_bounds__(256) void lin_dy_fix_kernel(const float* __restrict__ amax, int namax, const float* __restrict__ colpart, int nstat,
                                                         int N, float* __restrict__ cell, float* __restrict__ dbias) {
  __shared__ float wmax[4];
  __shared__ float psum[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (blockIdx.x == 0) {                                               // (uniform per workgroup)
    float am = 0.f;
    for (int i = threadIdx.x; i < namax; i += 256) am = fmaxf(am, amax[i]);
    for (int o = 32; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 64));
    if (lane == 0) wmax[wave] = am;
    __syncthreads();
    if (threadIdx.x == 0) {
      am = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
      const int field = (int)((__builtin_bit_cast(unsigned, am) >> 23) & 0xffu);
      int e = 0;
      if (am > 0.f && field != 255) {
        e = field - 127 - kLinGradExp;
        e = e < -126 ? -126 : (e > 126 ? 126 : e);
      }
      cell[0] = __builtin_bit_cast(float, (unsigned)(127 - e) << 23);
      cell[1] = __builtin_bit_cast(float, (unsigned)(127 + e) << 23);
    }
  }
  if (!dbias) return;                                                  // (uniform)
  const int n = blockIdx.x * 64 + lane;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (n < N) {
    int b = wave;
    for (; b + 12 < nstat; b += 16) {
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] += colpart[(long long)(b + 4 * q) * N + n];
    }
    for (int q = 0; b < nstat; b += 4, ++q) a[q] += colpart[(long long)b * N + n];
  }
  psum[wave][lane] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  if (wave == 0 && n < N) dbias[n] = ((psum[0][lane] + psum[1][lane]) + psum[2][lane]) + psum[3][lane];
}

// grid (kblocks, nblocks, chunks), block 256 = 2 x 2 waves of AT x BT tiles; xc / dc: COL images of x^ / dy^
template <int AT, int BT>
__global__ __launch_bounds__(256) void lin_wgrad_kernel(const char* __restrict__ xc, const char* __restrict__ dc, int KT, int NT, int MS,
                                                        int spc, int K, int N, float* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int kt0 = (blockIdx.x * 2 + (wave & 1)) * AT, nt0 = (blockIdx.y * 2 + (wave >> 1)) * BT;
  if (kt0 >= KT || nt0 >= NT) return;                                   // (no barrier in this kernel)
  const int s0 = blockIdx.z * spc, s1 = s0 + spc < MS ? s0 + spc : MS;
  const char* ap[AT];
  const char* bp[BT];
#pragma unroll
  for (int t = 0; t < AT; ++t) ap[t] = xc + ((long long)(kt0 + t < KT ? kt0 + t : KT - 1) * MS * 64 + lane) * 16;    // tiles behind the last one:
#pragma unroll
  for (int u = 0; u < BT; ++u) bp[u] = dc + ((long long)(nt0 + u < NT ? nt0 + u : NT - 1) * MS * 64 + lane) * 16;    // clamped, never stored
  f32x4 acc[AT][BT];
#pragma unroll
  for (int t = 0; t < AT; ++t)
#pragma unroll
    for (int u = 0; u < BT; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  f16x8 a[2][AT], b[2][BT];
  auto load = [&](const int buf, int s) {
#pragma unroll
    for (int t = 0; t < AT; ++t) a[buf][t] = *(const f16x8*)(ap[t] + (long long)s * 1024);
#pragma unroll
    for (int u = 0; u < BT; ++u) b[buf][u] = *(const f16x8*)(bp[u] + (long long)s * 1024);
  };
  auto compute = [&](const int buf) {                                    // A = x^ (rows k), B = dy^ (columns n): lane (li, g) owns
#pragma unroll                                                           // dW[n = li][k = 4 g .. 4 g + 3] of a tile pair
    for (int t = 0; t < AT; ++t)
#pragma unroll
      for (int u = 0; u < BT; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[buf][t], b[buf][u], acc[t][u], 0, 0, 0);
  };
  // one token step ahead; prefetches are unconditional at a clamped step (see gemm_kernel)
  load(0, s0);
  int s = s0;
  for (; s + 2 <= s1; s += 2) {
    load(1, s + 1);
    __builtin_amdgcn_sched_barrier(0);
    compute(0);
    __builtin_amdgcn_sched_barrier(0);
    load(0, s + 2 < s1 ? s + 2 : s1 - 1);
    __builtin_amdgcn_sched_barrier(0);
    compute(1);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (s < s1) compute(0);
  float* base = part + (long long)blockIdx.z * N * K;
#pragma unroll
  for (int t = 0; t < AT; ++t) {
    const int k = (kt0 + t) * 16 + 4 * g;
    if (kt0 + t >= KT || k >= K) continue;                               // K % 4 == 0: the quad is inside or outside
#pragma unroll
    for (int u = 0; u < BT; ++u) {
      const int n = (nt0 + u) * 16 + li;
      if (nt0 + u >= NT || n >= N) continue;
      *(float4*)(base + (long long)n * K + k) = make_float4(acc[t][u][0], acc[t][u][1], acc[t][u][2], acc[t][u][3]);
    }
  }
}

// dW quad = (part[0] + part[1] + ... in chunk order) * 2^e
__global__ __launch_bounds__(256) void lin_wgrad_reduce_kernel(const float* __restrict__ part, int chunks, long long quads,
                                                               const float* __restrict__ cell, float* __restrict__ dw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= quads) return;
  const float up = cell[1];
  float4 s = ((const float4*)part)[i];
  for (int c = 1; c < chunks; ++c) {
    const float4 v = ((const float4*)part)[(long long)c * quads + i];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  ((float4*)dw)[i] = make_float4(s.x * up, s.y * up, s.z * up, s.w * up);
}

template <bool ROWS, bool COLS>
hipError_t launch_image(const float* src, long long M, int C, int ld, int CT, int MS, const float* cell, void* rows, void* cols, hipStream_t st) {
  hipLaunchKernelGGL((lin_image_kernel<ROWS, COLS>), dim3((unsigned)MS, (unsigned)((C + 63) / 64)), dim3(256), 0, st, src, M, C, ld, CT, MS, cell,
                     (f16*)rows, (f16*)cols);
  return hipGetLastError();
}

}  // namespace

static size_t linear_train_scratch_bytes(long long M, int K, int N) {
  LinPlan p;
  return linear_plan(M, K, N, &p) ? p.bytes : 0;
}

static hipError_t launch_linear_forward(const float* x, const float* w, const float* bias, long long M, int K, int N, float* y, void* scratch,
                                        hipStream_t st) {
  LinPlan p;
  if (!linear_plan(M, K, N, &p)) return hipErrorInvalidValue;
  char* sc = (char*)scratch;
  hipError_t e = launch_pack_gemm(w, nullptr, nullptr, N, 0, 0, K, 0, 0, 0, p.NT, p.KS, sc + p.wpack, nullptr, st);
  if (e != hipSuccess) return e;
  if ((e = launch_image<true, false>(x, M, K, p.ldk, p.KT, p.MS, nullptr, sc + p.xrows, nullptr, st)) != hipSuccess) return e;
  if (bias && (e = launch_vec_place((float*)(sc + p.biaspad), bias, N, 0.f, st)) != hipSuccess) return e;   // whole tiles are read
  GemmParams g{};
  g.a_hi = sc + p.xrows; g.lda = p.ldk; g.M = (int)M; g.KS = p.KS;
  g.w_hi = sc + p.wpack; g.ntiles = p.NT; g.Nreal = N;
  g.bias = bias ? (const float*)(sc + p.biaspad) : nullptr;
  g.out = y; g.ldo = N;
  return launch_gemm(g, EPI_F32, st);
}

static hipError_t launch_linear_backward(const float* x, const float* w, const float* dy, long long M, int K, int N, float* dx, float* dw,
                                         float* dbias, void* scratch, hipStream_t st) {
  LinPlan p;
  if (!linear_plan(M, K, N, &p)) return hipErrorInvalidValue;
  char* sc = (char*)scratch;
  float* cell = (float*)(sc + p.cell);
  hipError_t e;
  const int gy = cdiv(N, 256);
  hipLaunchKernelGGL(lin_dy_stats_kernel, dim3(p.nstat, gy), dim3(256), 0, st, dy, M, N, p.stat_rows, (float*)(sc + p.amax), (float*)(sc + p.colpart));
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(lin_dy_fix_kernel, dim3((N + 63) / 64), dim3(256), 0, st, (const float*)(sc + p.amax), p.nstat * gy,
                     (const float*)(sc + p.colpart), p.nstat, N, cell, dbias);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (!dx && !dw) return hipSuccess;
  if (dx && dw) e = launch_image<true, true>(dy, M, N, p.ldn, p.NT, p.MS, cell, sc + p.dyrows, sc + p.dycol, st);
  else if (dx) e = launch_image<true, false>(dy, M, N, p.ldn, p.NT, p.MS, cell, sc + p.dyrows, nullptr, st);
  else e = launch_image<false, true>(dy, M, N, p.ldn, p.NT, p.MS, cell, nullptr, sc + p.dycol, st);
  if (e != hipSuccess) return e;
  if (dx) {
    const long long n = (long long)p.KT * p.NS * 64;
    hipLaunchKernelGGL(lin_pack_t_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, N, K, p.KT, p.NS, (f16*)(sc + p.wt));
    if ((e = hipGetLastError()) != hipSuccess) return e;
    GemmParams g{};
    g.a_hi = sc + p.dyrows; g.lda = p.ldn; g.M = (int)M; g.KS = p.NS;
    g.w_hi = sc + p.wt; g.ntiles = p.KT; g.Nreal = K;
    g.out = dx; g.ldo = K; g.scale = cell + 1;
    if ((e = launch_gemm(g, EPI_F32_SCALED, st)) != hipSuccess) return e;
  }
  if (dw) {
    if ((e = launch_image<false, true>(x, M, K, p.ldk, p.KT, p.MS, nullptr, nullptr, sc + p.xcol, st)) != hipSuccess) return e;
    hipLaunchKernelGGL((lin_wgrad_kernel<kLinAT, kLinBT>), dim3(p.kblocks, p.nblocks, p.chunks), dim3(256), 0, st, (const char*)(sc + p.xcol),
                       (const char*)(sc + p.dycol), p.KT, p.NT, p.MS, p.spc, K, N, (float*)(sc + p.part));
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const long long quads = (long long)N * K / 4;
    hipLaunchKernelGGL(lin_wgrad_reduce_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, (const float*)(sc + p.part), p.chunks,
                       quads, (const float*)cell, dw);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace amx

namespace {
using amx::fail;

// the envelope and the scratch of the two linear entries: AMX_OK or the refusal, before any launch
int linear_args_ok(const char* what, long long m, int k, int n, const void* d_scratch, size_t scratch_bytes) {
  const size_t need = amx::linear_train_scratch_bytes(m, k, n);
  if (need == 0)
    return fail(AMX_ERR_INVALID, "%s: (M, K, N) = (%lld, %d, %d) is outside the envelope (K, N multiples of 4 up to 2^20, M * max(K, N) < 2^31)",
                what, m, k, n);
  if (!d_scratch || scratch_bytes < need || ((uintptr_t)d_scratch & 15)) return fail(AMX_ERR_WORKSPACE, "%s scratch needs %zu bytes, 16-byte aligned", what, need);
  return AMX_OK;
}
bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return !(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15);
}
}  // namespace

extern "C" {

size_t amx_linear_train_scratch_bytes(long long m, int k, int n) { return amx::linear_train_scratch_bytes(m, k, n); }

int amx_linear(const float* d_x, const float* d_w, const float* d_b, int m, int k, int n, int split, float* d_y, void* stream) {
  if (!d_x || !d_w || !d_y) return fail(AMX_ERR_INVALID, "null argument");
  if (m < 1 || k < 1 || n < 4 || (n % 4) || k > 64 * 17) return fail(AMX_ERR_INVALID, "linear: m >= 1, 1 <= k <= 1088, n a multiple of 4 (got %d %d %d)", m, k, n);
  hipStream_t st = (hipStream_t)stream;
  auto up = [](int v, int mult) { return (v + mult - 1) / mult * mult; };
  const int kp = up(k, 32), ntiles = up(n, 16) / 16, KS = kp / 32;
  const size_t abytes = (size_t)m * kp * 2, wbytes = (size_t)ntiles * KS * 1024, bbytes = (size_t)ntiles * 16 * 4;
  char* buf = nullptr;
  AMX_HIP(hipMalloc((void**)&buf, 2 * abytes + 2 * wbytes + bbytes + 1024));
  char *a_hi = buf, *a_lo = buf + abytes, *w_hi = buf + 2 * abytes, *w_lo = w_hi + wbytes;
  float* bias = (float*)(w_lo + wbytes);
  int rc = AMX_OK;
  hipError_t e = amx::launch_ln_rows(d_x, 0, k, k, nullptr, nullptr, 0.f, m, m, m, 0, 0, a_hi, split ? a_lo : nullptr, kp, st);
  if (e == hipSuccess) e = amx::launch_pack_gemm(d_w, nullptr, nullptr, n, 0, 0, k, 0, 0, 0, ntiles, KS, w_hi, split ? w_lo : nullptr, st);
  if (e == hipSuccess) e = amx::launch_vec_place(bias, d_b, n, 0.f, st);
  if (e == hipSuccess && ntiles * 16 > n) e = amx::launch_vec_place(bias + n, nullptr, ntiles * 16 - n, 0.f, st);
  if (e == hipSuccess) {
    amx::GemmParams g{};
    g.a_hi = a_hi; g.a_lo = split ? a_lo : nullptr; g.lda = kp; g.M = m; g.KS = KS; g.w_hi = w_hi; g.w_lo = split ? w_lo : nullptr;
    g.ntiles = ntiles; g.Nreal = n; g.bias = bias; g.out = d_y; g.ldo = n;
    e = amx::launch_gemm(g, amx::EPI_F32, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) rc = fail(AMX_ERR_HIP, "linear: %s", hipGetErrorString(e));
  (void)hipFree(buf);
  return rc;
}

int amx_linear_forward(const float* d_x, const float* d_w, const float* d_bias, long long m, int k, int n, float* d_y, void* d_scratch,
                       size_t scratch_bytes, void* stream) {
  if (!d_x || !d_w || !d_y) return fail(AMX_ERR_INVALID, "linear forward: null argument");
  if (int rc = linear_args_ok("linear forward", m, k, n, d_scratch, scratch_bytes)) return rc;
  if (!aligned16(d_x, d_y)) return fail(AMX_ERR_INVALID, "linear forward: d_x and d_y must be 16-byte aligned");
  AMX_HIP(amx::launch_linear_forward(d_x, d_w, d_bias, m, k, n, d_y, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

int amx_linear_backward(const float* d_x, const float* d_w, const float* d_dy, long long m, int k, int n, float* d_dx, float* d_dw,
                        float* d_dbias, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (!d_x || !d_w || !d_dy) return fail(AMX_ERR_INVALID, "linear backward: null argument");
  if (int rc = linear_args_ok("linear backward", m, k, n, d_scratch, scratch_bytes)) return rc;
  if (!aligned16(d_x, d_dy, d_dx, d_dw)) return fail(AMX_ERR_INVALID, "linear backward: d_x, d_dy, d_dx and d_dw must be 16-byte aligned");
  AMX_HIP(amx::launch_linear_backward(d_x, d_w, d_dy, m, k, n, d_dx, d_dw, d_dbias, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

}  // extern "C"
