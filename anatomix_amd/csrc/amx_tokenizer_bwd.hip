// anatomix_amd -- the conv tokenizer of the 3D ViT (PatchEmbedDeeper: stem + three stride-2 residual stages, amx_tokenizer.hip) under
// autograd: a train-mode forward that keeps what the backward reads, and the backward for the 37 parameter gradients (no dx: the
// network input needs none).  `proj` stays a torch module; its input h3 is what the forward returns.
//
// Forward: the engine's kernels (tokstem / tokconv / tok_apply / tok_combine) on a plan of NON-aliased buffers inside `saved`:
//   per norm   mean, rstd [n][C] fp32 (tok_finalize_train: tok_finalize's double combine, plus the two statistics)
//   stem       h0 and its 2x2x2 average p0 as hi + lo f16 planes (the raw stem output is never stored: the backward recomputes it)
//   stage k    raw1, raw2, raws fp32 channels-last; a1, h(k+1) [, p(k+1)] as hi + lo planes
// Backward, per stage from the last to the first (d_h = gradient of the stage output, fp32):
//   tok_nadj_stats / _finalize   g = d_h * lrelu'(h) (the sign comes from the saved planes, hi + lo > 0); per (n, c) sums of g and g x^
//                                for norm2 and skip_norm in one pass, x^ = (raw - mean) rstd from the SAVED raw output (never by
//                                inverting the affine: gamma may be 0 or negative); per-block partials, combined in double -> d_gamma,
//                                d_beta and the coefficients of d_raw = gamma rstd (g - mean g - x^ mean(g x^))
//   tok_nadj_apply / tok_amax_fix / tok_split   d_raw fp32 and max |d_raw| per tensor -> one power of two per tensor on the device
//                                (2^e <= max / 8 < 2^(e+1), as amx_linear_backward) -> hi + lo f16 planes of d_raw 2^-e
//   tokwgrad<taps, stride>       dW[co][ci][tap] = sum_v d_raw[v][co] x[stride v + tap - 1][ci] (zero outside): the voxel is the
//                                reduction index of the MFMA, both operands gathered channel-wise from the channels-last planes;
//                                a wave owns one tap, 32 x 32 channels and a contiguous chunk of voxel steps; fp32 partials per chunk,
//                                added in chunk order in double (tok_wgrad_reduce) and multiplied by 2^e
//   stride-1 / 1x1 data gradient the forward conv kernel (tokconv) on the d_raw planes with flipped, transposed weights (tok_pack_t)
//   tokdgrad2                    the stride-2 data gradient per parity class of the INPUT voxel: an even coordinate meets tap 1 alone,
//                                an odd one taps 0 and 2, so a class has 1, 2, 4 or 8 live taps; tiles of 16 same-parity voxels; the
//                                epilogue adds the AvgPool adjoint of the skip branch (an eighth of the pooled voxel's gradient)
//   tokstem_bwd<pass>            the stem: the 1-channel conv is recomputed in fp32 on the vector ALUs (27 taps: more exact than the
//                                three f16 MFMAs of the forward, and 32x less traffic than a stored raw); pass 0 the norm sums,
//                                pass 1 d_raw and the 32 x 27 weight gradient
// Every product of two stored tensors uses hi + lo f16 operands and fp32 sums (three MFMAs); no float atomics; every long sum is
// per-block partials in a fixed order, combined in double: bit-identical run to run.  The bias of a conv that feeds an InstanceNorm
// has an exactly zero gradient (sum of d_raw over a sample is 0 for every channel); those seven outputs are written as zeros.
#include <string.h>

#include <algorithm>
#include <string>

#include "amx_device.h"
#include "amx_gemm.h"
#include "amx_launch.h"

namespace amx {

constexpr float kTokSlope = 0.01f;
constexpr int kTokGradExp = 3;              // max |d_raw 2^-e| lies in [2^3, 2^4)
constexpr int kNadjVox = 1024;              // voxels per workgroup of the norm-adjoint passes
constexpr int kStemVox = 2048;              // voxels per workgroup of tokstem_bwd
constexpr int kWgSteps = 64;                // 32-voxel steps per chunk of tokwgrad, at least
constexpr int kWgMaxChunks = 256;
constexpr int kTokC[4] = {32, 32, 64, 128}; // channels of h0 .. h3

static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
__device__ __forceinline__ float half_bits(unsigned short b) { return (float)__builtin_bit_cast(f16, b); }
__device__ __forceinline__ void split8f(const float (&v)[8], uint4& hi, uint4& lo) {
  unsigned short h[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const f16 a = (f16)v[e];
    h[e] = __builtin_bit_cast(unsigned short, a);
    l[e] = to_bits<f16>(v[e] - (float)a);
  }
  hi = make_uint4(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16), h[6] | ((unsigned)h[7] << 16));
  lo = make_uint4(l[0] | ((unsigned)l[1] << 16), l[2] | ((unsigned)l[3] << 16), l[4] | ((unsigned)l[5] << 16), l[6] | ((unsigned)l[7] << 16));
}

// =====================================================================================================================
// forward additions
// tok_finalize_kernel's arithmetic (same scale / shift bits), plus mean and rstd for the backward
__global__ __launch_bounds__(256) void tok_finalize_train_kernel(const float* __restrict__ stats, int slots, int C, double inv_count,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                 float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ mean_out,
                                                                 float* __restrict__ rstd_out) {
  __shared__ double ss[256], sq[256];
  const int n = blockIdx.x / C, c = blockIdx.x % C;
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < slots; i += 256) {
    const float2 v = *(const float2*)(stats + (((long long)n * slots + i) * C + c) * 2);
    s += v.x;
    q += v.y;
  }
  ss[threadIdx.x] = s;
  sq[threadIdx.x] = q;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { ss[threadIdx.x] += ss[threadIdx.x + o]; sq[threadIdx.x] += sq[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double mean = ss[0] * inv_count;
    double var = sq[0] * inv_count - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const double r = 1.0 / sqrt(var + (double)eps), k = (double)gamma[c] * r;
    scale[n * C + c] = (float)k;
    shift[n * C + c] = (float)((double)beta[c] - mean * k);
    mean_out[n * C + c] = (float)mean;
    rstd_out[n * C + c] = (float)r;
  }
}

// hi + lo planes [n][vox][C] -> fp32 [n][C][vox]; one thread = 8 channels of one voxel
__global__ __launch_bounds__(256) void tok_export_kernel(const char* __restrict__ hi, const char* __restrict__ lo, long long vox, int C,
                                                         long long total, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int cg = C / 8, c0 = (int)(i % cg) * 8;
  const long long nv = i / cg, n = nv / vox, v = nv - n * vox;
  const uint4 h = *(const uint4*)(hi + i * 16), l = *(const uint4*)(lo + i * 16);
  const unsigned hw[4] = {h.x, h.y, h.z, h.w}, lw[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const unsigned short hb = (unsigned short)(hw[e >> 1] >> (16 * (e & 1))), lb = (unsigned short)(lw[e >> 1] >> (16 * (e & 1)));
    out[(n * C + c0 + e) * vox + v] = half_bits(hb) + half_bits(lb);
  }
}

// =====================================================================================================================
// InstanceNorm (+ LeakyReLU) adjoint of one or two norms that share their incoming gradient
struct NadjParams {
  const float* d;               // gradient of the activation behind the LeakyReLU, element (n, v, c) at n sn + v sv + c sc
  long long sn, sv, sc;
  const float* dscale;          // one device float that multiplies d (the 2^e of the data gradient that produced it), or null
  const char* m_hi;             // that activation's saved planes [n][vox][C]: the sign mask is hi + lo > 0
  const char* m_lo;
  const float* rawa;            // saved raw conv outputs, fp32 [n][vox][C]; rawb null: one norm
  const float* rawb;
  const float* mra;             // mean [n][C], then rstd [n][C]
  const float* mrb;
  int N, C, nblk;
  long long vox;
  float* part;                  // stats: [n][nblk][C][3] = sums of g, g x^a, g x^b
  const float4* coefa;          // apply: per (n, c) {gamma rstd, mean g, mean(g x^), 0}
  const float4* coefb;
  float* outa;                  // apply: d_raw fp32 [n][vox][C]
  float* outb;
  float* amax;                  // apply: [n][nblk][2] max |d_raw|
};

// grid (nblk, N), block 256: thread = (voxel slot, channel quad); a workgroup walks kNadjVox voxels of one sample
template <bool APPLY>
__global__ __launch_bounds__(256) void tok_nadj_kernel(NadjParams p) {
  __shared__ float red[256][13];
  const int n = blockIdx.y, C = p.C, nq = C / 4, q = threadIdx.x % nq, vr = threadIdx.x / nq, R = 256 / nq, c0 = 4 * q;
  const long long v0 = (long long)blockIdx.x * kNadjVox, v1 = v0 + kNadjVox < p.vox ? v0 + kNadjVox : p.vox;
  const bool two = p.rawb != nullptr;
  const float ds = p.dscale ? *p.dscale : 1.f;
  float ma[4], ra[4], mb[4], rb[4];
  float4 ca[4], cb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ma[j] = p.mra[n * C + c0 + j]; ra[j] = p.mra[(p.N + n) * C + c0 + j];
    mb[j] = two ? p.mrb[n * C + c0 + j] : 0.f; rb[j] = two ? p.mrb[(p.N + n) * C + c0 + j] : 0.f;
    if (APPLY) { ca[j] = p.coefa[n * C + c0 + j]; cb[j] = two ? p.coefb[n * C + c0 + j] : make_float4(0.f, 0.f, 0.f, 0.f); }
  }
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2a[4] = {0.f, 0.f, 0.f, 0.f}, s2b[4] = {0.f, 0.f, 0.f, 0.f}, ama = 0.f, amb = 0.f;
  for (long long v = v0 + vr; v < v1; v += R) {
    const long long e = ((long long)n * p.vox + v) * C + c0;
    const uint2 mh = *(const uint2*)(p.m_hi + e * 2), ml = *(const uint2*)(p.m_lo + e * 2);
    const unsigned hw[2] = {mh.x, mh.y}, lw[2] = {ml.x, ml.y};
    const float4 xa4 = *(const float4*)(p.rawa + e);
    const float4 xb4 = two ? *(const float4*)(p.rawb + e) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float xa[4] = {xa4.x, xa4.y, xa4.z, xa4.w}, xb[4] = {xb4.x, xb4.y, xb4.z, xb4.w};
    float oa[4], ob[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float act = half_bits((unsigned short)(hw[j >> 1] >> (16 * (j & 1)))) + half_bits((unsigned short)(lw[j >> 1] >> (16 * (j & 1))));
      const float dv = p.d[n * p.sn + v * p.sv + (c0 + j) * p.sc] * ds;
      const float g = act > 0.f ? dv : dv * kTokSlope;
      const float ha = (xa[j] - ma[j]) * ra[j], hb = (xb[j] - mb[j]) * rb[j];
      if (!APPLY) {
        s1[j] += g; s2a[j] += g * ha; s2b[j] += g * hb;
      } else {
        oa[j] = ca[j].x * (g - ca[j].y - ha * ca[j].z);
        ob[j] = cb[j].x * (g - cb[j].y - hb * cb[j].z);
        ama = fmaxf(ama, fabsf(oa[j])); amb = fmaxf(amb, fabsf(ob[j]));
      }
    }
    if (APPLY) {
      *(float4*)(p.outa + e) = make_float4(oa[0], oa[1], oa[2], oa[3]);
      if (two) *(float4*)(p.outb + e) = make_float4(ob[0], ob[1], ob[2], ob[3]);
    }
  }
  if (!APPLY) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { red[threadIdx.x][j] = s1[j]; red[threadIdx.x][4 + j] = s2a[j]; red[threadIdx.x][8 + j] = s2b[j]; }
    __syncthreads();
    if ((int)threadIdx.x < C) {                        // channel c: the R voxel slots in slot order
      const int c = threadIdx.x, qq = c >> 2, j = c & 3;
      float t0 = 0.f, t1 = 0.f, t2 = 0.f;
      for (int r = 0; r < R; ++r) { t0 += red[r * nq + qq][j]; t1 += red[r * nq + qq][4 + j]; t2 += red[r * nq + qq][8 + j]; }
      float* o = p.part + (((long long)n * p.nblk + blockIdx.x) * C + c) * 3;
      o[0] = t0; o[1] = t1; o[2] = t2;
    }
  } else {
    red[threadIdx.x][0] = ama; red[threadIdx.x][1] = amb;
    __syncthreads();
    if (threadIdx.x < 2) {
      float m = 0.f;
      for (int r = 0; r < 256; ++r) m = fmaxf(m, red[r][threadIdx.x]);
      p.amax[((long long)n * p.nblk + blockIdx.x) * 2 + threadIdx.x] = m;
    }
  }
}

// one workgroup per channel: partials -> (double) sums per sample -> coefficients; d_gamma, d_beta summed over the samples in order
__global__ __launch_bounds__(256) void tok_nadj_finalize_kernel(const float* __restrict__ part, int N, int nblk, int C, double inv_vox,
                                                                const float* __restrict__ gamma_a, const float* __restrict__ mra,
                                                                const float* __restrict__ gamma_b, const float* __restrict__ mrb,
                                                                float4* __restrict__ coefa, float4* __restrict__ coefb, float* __restrict__ dga,
                                                                float* __restrict__ dba, float* __restrict__ dgb, float* __restrict__ dbb) {
  __shared__ double sh[3][256];
  const int c = blockIdx.x;
  double g1 = 0.0, g2a = 0.0, g2b = 0.0;
  for (int n = 0; n < N; ++n) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += 256) {
      const float* o = part + (((long long)n * nblk + i) * C + c) * 3;
      s[0] += o[0]; s[1] += o[1]; s[2] += o[2];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 3; ++j) sh[j][threadIdx.x] = s[j];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o)
#pragma unroll
        for (int j = 0; j < 3; ++j) sh[j][threadIdx.x] += sh[j][threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      g1 += sh[0][0]; g2a += sh[1][0]; g2b += sh[2][0];
      const float m1 = (float)(sh[0][0] * inv_vox);
      coefa[n * C + c] = make_float4(gamma_a[c] * mra[(N + n) * C + c], m1, (float)(sh[1][0] * inv_vox), 0.f);
      if (coefb) coefb[n * C + c] = make_float4(gamma_b[c] * mrb[(N + n) * C + c], m1, (float)(sh[2][0] * inv_vox), 0.f);
    }
  }
  if (threadIdx.x == 0) {
    if (dga) dga[c] = (float)g2a;
    if (dba) dba[c] = (float)g1;
    if (dgb) dgb[c] = (float)g2b;
    if (dbb) dbb[c] = (float)g1;
  }
}

// grid 2 (tensor a, b), block 256: max |d_raw| -> cell {2^-e, 2^e}; an all-zero tensor takes e = 0
__global__ __launch_bounds__(256) void tok_amax_fix_kernel(const float* __restrict__ amax, int count, float* __restrict__ cell_a,
                                                           float* __restrict__ cell_b) {
  __shared__ float wmax[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float am = 0.f;
  for (int i = threadIdx.x; i < count; i += 256) am = fmaxf(am, amax[(long long)i * 2 + blockIdx.x]);
  for (int o = 32; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 64));
  if (lane == 0) wmax[wave] = am;
  __syncthreads();
  if (threadIdx.x == 0) {
    am = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    const int field = (int)((__builtin_bit_cast(unsigned, am) >> 23) & 0xffu);
    int e = 0;
    if (am > 0.f && field != 255) {
      e = field - 127 - kTokGradExp;
      e = e < -126 ? -126 : (e > 126 ? 126 : e);
    }
    float* cell = blockIdx.x ? cell_b : cell_a;
    if (cell) {
      cell[0] = __builtin_bit_cast(float, (unsigned)(127 - e) << 23);
      cell[1] = __builtin_bit_cast(float, (unsigned)(127 + e) << 23);
    }
  }
}

// fp32 [total 8-channel groups] times cell[0] -> hi + lo planes
__global__ __launch_bounds__(256) void tok_split_kernel(const float* __restrict__ src, const float* __restrict__ cell, long long total,
                                                        char* __restrict__ hi, char* __restrict__ lo) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float s = cell[0];
  const float4 a = *(const float4*)(src + i * 8), b = *(const float4*)(src + i * 8 + 4);
  const float v[8] = {a.x * s, a.y * s, a.z * s, a.w * s, b.x * s, b.y * s, b.z * s, b.w * s};
  uint4 h, l;
  split8f(v, h, l);
  *(uint4*)(hi + i * 16) = h;
  *(uint4*)(lo + i * 16) = l;
}

// conv weight [Cout][Cin][taps] -> the fragments of its TRANSPOSE (rows = input channels, reduction = output channels):
// [Cin / 16][tap * (Cout / 32) + chunk][lane][8], hi and lo; flip: tap t of the result is tap taps - 1 - t of the weight
__global__ void tok_pack_t_kernel(const float* __restrict__ w, int Cout, int Cin, int taps, int flip, f16* __restrict__ hi, f16* __restrict__ lo) {
  const int nch = Cout / 32, KS = taps * nch;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)(Cin / 16) * KS * 64) return;
  const int lane = idx & 63, ks = (idx >> 6) % KS, nt = (idx >> 6) / KS;
  const int tap = ks / nch, ch = ks % nch, n = nt * 16 + (lane & 15), c0 = ch * 32 + (lane >> 4) * 8;
  const int src_tap = flip ? taps - 1 - tap : tap;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = w[((long long)(c0 + e) * Cin + n) * taps + src_tap];
  uint4 h, l;
  split8f(v, h, l);
  ((uint4*)hi)[idx] = h;
  ((uint4*)lo)[idx] = l;
}

// =====================================================================================================================
// stride-2 data gradient, one parity class of the input voxel per blockIdx.z (+ the AvgPool adjoint of the skip branch)
struct TokDgrad2Params {
  const char* d_hi;             // d_raw 2^-e planes at the conv's OUTPUT extent [N][Do][Ho][Wo][Cout]
  const char* d_lo;
  int N, Do, Ho, Wo, Cout, Cin;
  const char* w_hi;             // tok_pack_t (no flip): [Cin / 16][27 * Cout / 32][64][8]
  const char* w_lo;
  const float* scale;           // 2^e of the planes
  const float* dpool;           // gradient of the pooled stage input, fp32 [N][Do][Ho][Wo][Cin], times 1 / *pscale
  const float* pscale;
  float* out;                   // fp32 [N][2 Do][2 Ho][2 Wo][Cin]
};

// grid (row blocks, Cin / (16 NT), 8), block 256 = 4 waves; a wave owns MT tiles of 16 consecutive voxels of the HALF-resolution raster:
// input voxel (2 z + pz, 2 y + py, 2 x + px).  Along an axis an even coordinate 2 j is read by output j through tap 1; an odd one,
// 2 j + 1, by output j + 1 through tap 0 (none at the far border) and by output j through tap 2.
template <int MT, int NT>
__global__ __launch_bounds__(256) void tokdgrad2_kernel(TokDgrad2Params p) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int wid = blockIdx.x * 4 + wave;
  const long long tiles = (long long)p.N * p.Do * p.Ho * p.Wo / 16;
  if ((long long)wid * MT >= tiles) return;
  const int pz = blockIdx.z >> 2, py = (blockIdx.z >> 1) & 1, px = blockIdx.z & 1;
  const int nt0 = blockIdx.y * NT, nch = p.Cout / 32, KS = 27 * nch;
  int tb[MT], tz[MT], ty[MT], tx[MT];
#pragma unroll
  for (int u = 0; u < MT; ++u) {
    const long long m = ((long long)wid * MT + u) * 16 + li;
    tx[u] = (int)(m % p.Wo);
    const long long r1 = m / p.Wo;
    ty[u] = (int)(r1 % p.Ho);
    const long long r2 = r1 / p.Ho;
    tz[u] = (int)(r2 % p.Do);
    tb[u] = (int)(r2 / p.Do);
  }
  const long long lo_off = p.d_lo - p.d_hi, wlo_off = p.w_lo - p.w_hi;
  f32x4 acc[NT][MT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int u = 0; u < MT; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int az = 0; az <= pz; ++az)
    for (int ay = 0; ay <= py; ++ay)
      for (int ax = 0; ax <= px; ++ax) {
        const int kz = pz ? 2 * az : 1, ky = py ? 2 * ay : 1, kx = px ? 2 * ax : 1;     // tap 0 comes with output j + 1
        const int oz = pz && !az, oy = py && !ay, ox = px && !ax;
        const int tap = kz * 9 + ky * 3 + kx;
        for (int ch = 0; ch < nch; ++ch) {
          const int ksl = tap * nch + ch;
          f16x8 wh[NT], wl[NT], xh[MT], xl[MT];
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const char* wp = p.w_hi + (((long long)(nt0 + t) * KS + ksl) * 64 + lane) * 16;
            wh[t] = *(const f16x8*)wp;
            wl[t] = *(const f16x8*)(wp + wlo_off);
          }
#pragma unroll
          for (int u = 0; u < MT; ++u) {
            const int iz = tz[u] + oz, iy = ty[u] + oy, ix = tx[u] + ox;
            const bool ok = iz < p.Do && iy < p.Ho && ix < p.Wo;
            const long long vox = (((long long)tb[u] * p.Do + iz) * p.Ho + iy) * p.Wo + ix;
            const char* src = p.d_hi + (vox * p.Cout + ch * 32 + g * 8) * 2;
            const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            xh[u] = ok ? *(const f16x8*)src : z;
            xl[u] = ok ? *(const f16x8*)(src + lo_off) : z;
          }
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int u = 0; u < MT; ++u) {
              acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], xh[u], acc[t][u], 0, 0, 0);
              acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], xl[u], acc[t][u], 0, 0, 0);
              acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[t], xh[u], acc[t][u], 0, 0, 0);
            }
        }
      }
  // lane (li, g) holds input channels n .. n + 3 of voxel li of every tile
  const float s = *p.scale, ps = 0.125f * *p.pscale;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = (nt0 + t) * 16 + 4 * g;
#pragma unroll
    for (int u = 0; u < MT; ++u) {
      const long long m = ((long long)wid * MT + u) * 16 + li;
      const float4 dp = *(const float4*)(p.dpool + m * p.Cin + n);
      const long long vox = (((long long)tb[u] * (2 * p.Do) + 2 * tz[u] + pz) * (2 * p.Ho) + 2 * ty[u] + py) * (2 * p.Wo) + 2 * tx[u] + px;
      *(float4*)(p.out + vox * p.Cin + n) =
          make_float4(acc[t][u][0] * s + dp.x * ps, acc[t][u][1] * s + dp.y * ps, acc[t][u][2] * s + dp.z * ps, acc[t][u][3] * s + dp.w * ps);
    }
  }
}

// =====================================================================================================================
// weight gradient: the voxel is the reduction index
struct TokWgradParams {
  const char* d_hi;             // d_raw 2^-e planes [N][Do][Ho][Wo][Cout]
  const char* d_lo;
  int N, Do, Ho, Wo, Cout;
  const char* x_hi;             // the conv's input planes [N][D][H][W][Cin]
  const char* x_lo;
  int D, H, W, Cin;
  int steps, spc, chunks;       // 32-voxel steps in all, per chunk; chunks
  float* part;                  // [chunks][Cout][Cin][TAPS]
};

// grid (ceil(chunks / 4), (Cout / 32) (Cin / 32), TAPS), block 256 = 4 waves, one chunk each.  Lane (li, g) of an operand fragment holds
// channel li of the eight voxels 32 step + 8 g .. + 7 (16-bit gathers from the channels-last planes; zero outside the volume).
template <int TAPS, int STRIDE>
__global__ __launch_bounds__(256) void tokwgrad_kernel(TokWgradParams p) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int chunk = blockIdx.x * 4 + wave;
  if (chunk >= p.chunks) return;
  const int nci = p.Cin / 32, co0 = (blockIdx.y / nci) * 32, ci0 = (blockIdx.y % nci) * 32, tap = blockIdx.z;
  const int kz = TAPS == 1 ? 1 : tap / 9, ky = TAPS == 1 ? 1 : (tap / 3) % 3, kx = TAPS == 1 ? 1 : tap % 3;
  const int s0 = chunk * p.spc, s1 = s0 + p.spc < p.steps ? s0 + p.spc : p.steps;
  const unsigned short* dh = (const unsigned short*)p.d_hi;
  const unsigned short* dl = (const unsigned short*)p.d_lo;
  const unsigned short* xh = (const unsigned short*)p.x_hi;
  const unsigned short* xl = (const unsigned short*)p.x_lo;
  f32x4 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
  for (int s = s0; s < s1; ++s) {
    long long m = (long long)s * 32 + 8 * g;
    int x = (int)(m % p.Wo);
    long long r = m / p.Wo;
    int y = (int)(r % p.Ho);
    r /= p.Ho;
    int z = (int)(r % p.Do), b = (int)(r / p.Do);
    u16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const long long dv = (m + e) * p.Cout + co0 + li;
      ah[0][e] = dh[dv]; ah[1][e] = dh[dv + 16];
      al[0][e] = dl[dv]; al[1][e] = dl[dv + 16];
      const int iz = z * STRIDE + kz - 1, iy = y * STRIDE + ky - 1, ix = x * STRIDE + kx - 1;
      const bool ok = iz >= 0 && iz < p.D && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      const long long xv = ((((long long)b * p.D + iz) * p.H + iy) * p.W + ix) * p.Cin + ci0 + li;
      bh[0][e] = ok ? xh[xv] : (unsigned short)0; bh[1][e] = ok ? xh[xv + 16] : (unsigned short)0;
      bl[0][e] = ok ? xl[xv] : (unsigned short)0; bl[1][e] = ok ? xl[xv + 16] : (unsigned short)0;
      if (++x == p.Wo) {                                   // the next voxel in raster order (a step may wrap rows, planes, samples)
        x = 0;
        if (++y == p.Ho) {
          y = 0;
          if (++z == p.Do) { z = 0; ++b; }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const f16x8 a_h = __builtin_bit_cast(f16x8, ah[t]), a_l = __builtin_bit_cast(f16x8, al[t]);
        const f16x8 b_h = __builtin_bit_cast(f16x8, bh[u]), b_l = __builtin_bit_cast(f16x8, bl[u]);
        acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_h, b_h, acc[t][u], 0, 0, 0);
        acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_h, b_l, acc[t][u], 0, 0, 0);
        acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_l, b_h, acc[t][u], 0, 0, 0);
      }
  }
  // lane (li, g) holds dW[co = 16 t + 4 g + j][ci = 16 u + li]
  float* base = p.part + (long long)chunk * p.Cout * p.Cin * TAPS;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        base[((long long)(co0 + 16 * t + 4 * g + j) * p.Cin + ci0 + 16 * u + li) * TAPS + tap] = acc[t][u][j];
}

// dW[i] = (sum over the chunks in index order, in double) * cell[1] (cell null: 1)
__global__ __launch_bounds__(256) void tok_wgrad_reduce_kernel(const float* __restrict__ part, int chunks, long long count,
                                                               const float* __restrict__ cell, float* __restrict__ dw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += (double)part[(long long)c * count + i];
  dw[i] = (float)(s * (cell ? (double)cell[1] : 1.0));
}

// =====================================================================================================================
// stem backward.  grid (nblk, N), block 256 = 32 voxel slots x 8 channel quads; a workgroup walks kStemVox voxels of one sample.
struct TokStemBwdParams {
  const float* x;               // [N][D][H][W]
  int N, D, H, W, nblk;
  const float* w;               // [32][27]
  const float* bias;            // [32]
  const float* mr;              // mean [N][32], rstd [N][32]
  const float* dh;              // gradient of h0, fp32 [N][D][H][W][32]
  const char* m_hi;             // h0 planes (sign mask)
  const char* m_lo;
  float* part;                  // pass 0: [n][nblk][32][3] (third sum unused: 0)
  const float4* coef;           // pass 1: per (n, c) {gamma rstd, mean g, mean(g x^), 0}
  float* wpart;                 // pass 1: [n nblk][32][27]
};

template <int PASS>
__global__ __launch_bounds__(256) void tokstem_bwd_kernel(TokStemBwdParams p) {
  __shared__ float4 ws[27][8];                         // [tap][channel quad]
  __shared__ float red[4][8][PASS == 0 ? 8 : 108];
  const int tid = threadIdx.x, q = tid & 7, vs = tid >> 3, n = blockIdx.y, c0 = 4 * q;
  for (int i = tid; i < 27 * 8; i += 256) {
    const int t = i >> 3, qq = i & 7;
    ws[t][qq] = make_float4(p.w[(4 * qq) * 27 + t], p.w[(4 * qq + 1) * 27 + t], p.w[(4 * qq + 2) * 27 + t], p.w[(4 * qq + 3) * 27 + t]);
  }
  __syncthreads();
  const long long vox = (long long)p.D * p.H * p.W, v0 = (long long)blockIdx.x * kStemVox, v1 = v0 + kStemVox < vox ? v0 + kStemVox : vox;
  float bias[4], mean[4], rstd[4];
  float4 cf[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bias[j] = p.bias[c0 + j]; mean[j] = p.mr[n * 32 + c0 + j]; rstd[j] = p.mr[(p.N + n) * 32 + c0 + j];
    if (PASS == 1) cf[j] = p.coef[n * 32 + c0 + j];
  }
  const float* xb = p.x + (long long)n * vox;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  float acc[PASS == 1 ? 4 : 1][27];
#pragma unroll
  for (int j = 0; j < (PASS == 1 ? 4 : 1); ++j)
#pragma unroll
    for (int t = 0; t < 27; ++t) acc[j][t] = 0.f;
  for (long long v = v0 + vs; v < v1; v += 32) {
    const int x = (int)(v % p.W), y = (int)(v / p.W % p.H), z = (int)(v / ((long long)p.W * p.H));
    float xt[27];
#pragma unroll
    for (int t = 0; t < 27; ++t) {
      const int iz = z + t / 9 - 1, iy = y + (t / 3) % 3 - 1, ix = x + t % 3 - 1;
      const bool ok = iz >= 0 && iz < p.D && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      xt[t] = ok ? xb[((long long)iz * p.H + iy) * p.W + ix] : 0.f;
    }
    float raw[4] = {bias[0], bias[1], bias[2], bias[3]};
#pragma unroll
    for (int t = 0; t < 27; ++t) {
      const float4 w4 = ws[t][q];
      raw[0] = fmaf(w4.x, xt[t], raw[0]); raw[1] = fmaf(w4.y, xt[t], raw[1]);
      raw[2] = fmaf(w4.z, xt[t], raw[2]); raw[3] = fmaf(w4.w, xt[t], raw[3]);
    }
    const long long e = ((long long)n * vox + v) * 32 + c0;
    const uint2 mh = *(const uint2*)(p.m_hi + e * 2), ml = *(const uint2*)(p.m_lo + e * 2);
    const unsigned hw[2] = {mh.x, mh.y}, lw[2] = {ml.x, ml.y};
    const float4 d4 = *(const float4*)(p.dh + e);
    const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float act = half_bits((unsigned short)(hw[j >> 1] >> (16 * (j & 1)))) + half_bits((unsigned short)(lw[j >> 1] >> (16 * (j & 1))));
      const float gg = act > 0.f ? dv[j] : dv[j] * kTokSlope;
      const float xh = (raw[j] - mean[j]) * rstd[j];
      if (PASS == 0) {
        s1[j] += gg; s2[j] += gg * xh;
      } else {
        const float dr = cf[j].x * (gg - cf[j].y - xh * cf[j].z);
#pragma unroll
        for (int t = 0; t < 27; ++t) acc[j][t] = fmaf(dr, xt[t], acc[j][t]);
      }
    }
  }
  // the 32 voxel slots of a quad: 8 within the wave (lanes 8 apart: fixed butterfly), then the 4 waves in order
  const int wave = tid >> 6, lane = tid & 63;
  auto slot_sum = [](float v) {
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
  };
  if (PASS == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = slot_sum(s1[j]), b = slot_sum(s2[j]);
      if (lane < 8) { red[wave][q][j] = a; red[wave][q][4 + j] = b; }
    }
    __syncthreads();
    if (tid < 32) {
      const int qq = tid >> 2, j = tid & 3;
      float* o = p.part + (((long long)n * p.nblk + blockIdx.x) * 32 + tid) * 3;
      o[0] = ((red[0][qq][j] + red[1][qq][j]) + red[2][qq][j]) + red[3][qq][j];
      o[1] = ((red[0][qq][4 + j] + red[1][qq][4 + j]) + red[2][qq][4 + j]) + red[3][qq][4 + j];
      o[2] = 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < 27; ++t) {
        const float a = slot_sum(acc[j][t]);
        if (lane < 8) red[wave][q][j * 27 + t] = a;
      }
    __syncthreads();
    float* o = p.wpart + ((long long)n * p.nblk + blockIdx.x) * 32 * 27;
    for (int i = tid; i < 32 * 27; i += 256) {
      const int c = i / 27, t = i - c * 27, qq = c >> 2, k = (c & 3) * 27 + t;
      o[i] = ((red[0][qq][k] + red[1][qq][k]) + red[2][qq][k]) + red[3][qq][k];
    }
  }
}

// =====================================================================================================================
// plans
namespace {

struct TrainPlan {
  int n, D[4], H[4], W[4];
  long long vox[4];                                   // voxels per sample at level k (extent >> k)
  // saved
  size_t mr[10];                                      // norm i: mean [n][C] then rstd [n][C]; 0 stem, 1 + 3 k norm1, 2 + 3 k norm2, 3 + 3 k skip_norm
  size_t h_hi[4], h_lo[4], p_hi[3], p_lo[3];          // h_k (level k, kTokC[k] channels); p_k = its 2x2x2 average (level k + 1)
  size_t raw1[3], raw2[3], raws[3], a1_hi[3], a1_lo[3];
  size_t saved_bytes;
  // forward scratch
  size_t f_stem_w, f_c1[3], f_c2[3], f_sk[3], f_stats, f_sc[3], f_sh[3], fwd_bytes;
  // backward scratch
  size_t b_cell, b_part, b_coefa, b_coefb, b_amax, b_fa, b_fb, b_pa_hi, b_pa_lo, b_pb_hi, b_pb_lo, b_dpool, b_dh[3], b_wt, b_wpart, bwd_bytes;
};

int wgrad_chunks(long long total_vox, int* spc_out) {
  const int steps = (int)(total_vox / 32);
  int chunks = cdiv(steps, kWgSteps);
  if (chunks > kWgMaxChunks) chunks = kWgMaxChunks;
  const int spc = cdiv(steps, chunks);
  *spc_out = spc;
  return cdiv(steps, spc);
}

bool train_plan(int n, int D, int H, int W, TrainPlan* out) {
  if (n < 1 || D < 8 || H < 8 || W < 16 || (W % 16) || (D % 8) || (H % 8)) return false;      // D, H, W even at levels 0 .. 2; stem rows of 16
  const long long tokens = (long long)(D / 8) * (H / 8) * (W / 8);
  if (tokens % 64) return false;
  // 2 x 128^3: beyond it the 64- and 128-channel stages would take tokconv's 64-voxel waves, instances no test of this route reaches
  if ((long long)n * D * H * W > (1LL << 22) || n > 65535) return false;
  TrainPlan p{};
  p.n = n;
  for (int k = 0; k < 4; ++k) { p.D[k] = D >> k; p.H[k] = H >> k; p.W[k] = W >> k; p.vox[k] = (long long)p.D[k] * p.H[k] * p.W[k]; }
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
  auto planes = [&](int level, int C, size_t& hi, size_t& lo) { hi = take((size_t)n * p.vox[level] * C * 2); lo = take((size_t)n * p.vox[level] * C * 2); };
  p.mr[0] = take((size_t)2 * n * 32 * 4);
  for (int k = 0; k < 3; ++k)
    for (int i = 1; i <= 3; ++i) p.mr[i + 3 * k] = take((size_t)2 * n * kTokC[k + 1] * 4);
  planes(0, 32, p.h_hi[0], p.h_lo[0]);
  for (int k = 0; k < 3; ++k) {
    const int cin = kTokC[k], cout = kTokC[k + 1];
    planes(k + 1, cin, p.p_hi[k], p.p_lo[k]);
    p.raw1[k] = take((size_t)n * p.vox[k + 1] * cout * 4);
    p.raw2[k] = take((size_t)n * p.vox[k + 1] * cout * 4);
    p.raws[k] = take((size_t)n * p.vox[k + 1] * cout * 4);
    planes(k + 1, cout, p.a1_hi[k], p.a1_lo[k]);
    planes(k + 1, cout, p.h_hi[k + 1], p.h_lo[k + 1]);
  }
  p.saved_bytes = o;
  // forward scratch: packed weights (hi then lo), statistic slots, three (scale, shift) sets
  o = 0;
  p.f_stem_w = take(2 * 2048);
  size_t wmax = 0;
  for (int k = 0; k < 3; ++k) {
    const int cin = kTokC[k], cout = kTokC[k + 1];
    const size_t b1 = (size_t)(cout / 16) * 27 * (cin / 32) * 1024, b2 = (size_t)(cout / 16) * 27 * (cout / 32) * 1024, bs = (size_t)(cout / 16) * (cin / 32) * 1024;
    p.f_c1[k] = take(2 * b1); p.f_c2[k] = take(2 * b2); p.f_sk[k] = take(2 * bs);
    wmax = std::max(wmax, std::max(b1, b2));
  }
  size_t slots = (size_t)(D / 2) * (H / 2) * 32;                                               // stem: a slot per row pair
  for (int k = 0; k < 3; ++k) slots = std::max(slots, (size_t)(p.vox[k + 1] / 32) * kTokC[k + 1]);   // convs: a slot per wave of >= 32 voxels
  p.f_stats = take((size_t)n * slots * 2 * 4);
  for (int i = 0; i < 3; ++i) { p.f_sc[i] = take((size_t)n * 128 * 4); p.f_sh[i] = take((size_t)n * 128 * 4); }
  p.fwd_bytes = o;
  // backward scratch
  o = 0;
  p.b_cell = take(16 * 256);
  size_t part = (size_t)n * cdiv(p.vox[0], kStemVox) * 32 * 3 * 4, amax = 8, felems = 0, wpart = (size_t)n * cdiv(p.vox[0], kStemVox) * 32 * 27 * 4;
  for (int k = 0; k < 3; ++k) {
    const int cin = kTokC[k], cout = kTokC[k + 1], nblk = cdiv(p.vox[k + 1], kNadjVox);
    part = std::max(part, (size_t)n * nblk * cout * 3 * 4);
    amax = std::max(amax, (size_t)n * nblk * 2 * 4);
    felems = std::max(felems, (size_t)((long long)n * p.vox[k + 1] * cout));
    int spc;
    const int chunks = wgrad_chunks((long long)n * p.vox[k + 1], &spc);
    wpart = std::max(wpart, (size_t)chunks * cout * std::max(cin, cout) * 27 * 4);
  }
  p.b_part = take(part);
  p.b_coefa = take((size_t)n * 128 * 16); p.b_coefb = take((size_t)n * 128 * 16);
  p.b_amax = take(amax);
  p.b_fa = take(felems * 4); p.b_fb = take(felems * 4);
  p.b_pa_hi = take(felems * 2); p.b_pa_lo = take(felems * 2); p.b_pb_hi = take(felems * 2); p.b_pb_lo = take(felems * 2);
  p.b_dpool = take(felems * 4);
  for (int k = 0; k < 3; ++k) p.b_dh[k] = take((size_t)n * p.vox[k] * kTokC[k] * 4);
  p.b_wt = take(2 * wmax);
  p.b_wpart = take(wpart);
  p.bwd_bytes = o;
  *out = p;
  return true;
}

// parameter slots (torch layouts): 0 stem conv w, 1 b, 2 norm w, 3 b; stage k at 4 + 11 k: conv1 w, b, norm1 w, b, conv2 w, b, norm2 w, b,
// skip w, skip_norm w, b
enum { S_C1W = 0, S_C1B, S_N1W, S_N1B, S_C2W, S_C2B, S_N2W, S_N2B, S_SKW, S_SNW, S_SNB, S_COUNT };
constexpr int kTokParams = 4 + 3 * S_COUNT;

// One walk states what the route launches: `go` false formats the launch report only (no pointer is dereferenced, nothing is launched).
struct Walk {
  const TrainPlan& P;
  hipStream_t st;
  bool go;
  std::string* log;
  VitLaunchInfo li{};

  hipError_t note(hipError_t e) {
    if (log && e == hipSuccess) { log->append(li.name); log->push_back('\n'); }
    return e;
  }
  hipError_t named(const char* name, hipError_t e) {
    li.report("%s", name);
    return note(e);
  }
  hipError_t last() { return go ? hipGetLastError() : hipSuccess; }
  hipError_t conv(const TokConvParams& cp, int taps, int stride) {
    if (!go) {
      tokconv_report(cp, taps, stride, &li);
      return note(hipSuccess);
    }
    return note(launch_tokconv(cp, taps, stride, st, &li));
  }
  TokConvParams conv_params(const char* x_hi, const char* x_lo, int lvl_in, int Cin, int stride, int Cout, const char* w, size_t wbytes, const float* bias,
                            float* raw, float* stats) const {
    TokConvParams cp{};
    cp.x_hi = x_hi; cp.x_lo = x_lo; cp.N = P.n; cp.D = P.D[lvl_in]; cp.H = P.H[lvl_in]; cp.W = P.W[lvl_in]; cp.Cin = Cin;
    cp.Do = cp.D / stride; cp.Ho = cp.H / stride; cp.Wo = cp.W / stride; cp.Cout = Cout;
    cp.w_hi = w; cp.w_lo = w + wbytes; cp.bias = bias; cp.raw = raw; cp.stats = stats;
    return cp;
  }

  // ---- forward
  hipError_t finalize(const float* stats, int slots, int C, long long count, const float* gamma, const float* beta, float eps, float* sc, float* sh,
                      float* mr) {
    if (go) hipLaunchKernelGGL(tok_finalize_train_kernel, dim3(P.n * C), dim3(256), 0, st, stats, slots, C, 1.0 / (double)count, gamma, beta, eps, sc, sh,
                               mr, mr + (size_t)P.n * C);
    return named("tok_finalize_train", last());
  }
  hipError_t exported(const char* hi, const char* lo, int level, int C, float* out) {
    const long long total = (long long)P.n * P.vox[level] * C / 8;
    if (go) hipLaunchKernelGGL(tok_export_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, hi, lo, P.vox[level], C, total, out);
    return named("tok_export", last());
  }
  hipError_t forward(const float* x, const float* const* prm, float eps, float* out_h3, char* sv, char* sc) {
    hipError_t e;
#define AMX_W(expr) do { if ((e = (expr)) != hipSuccess) return e; } while (0)
    const int n = P.n;
    float* stats = (float*)(sc + P.f_stats);
    float *sc0 = (float*)(sc + P.f_sc[0]), *sh0 = (float*)(sc + P.f_sh[0]), *sc1 = (float*)(sc + P.f_sc[1]), *sh1 = (float*)(sc + P.f_sh[1]);
    float *sc2 = (float*)(sc + P.f_sc[2]), *sh2 = (float*)(sc + P.f_sh[2]);
    auto param = [&](int i) { return go ? prm[i] : (const float*)nullptr; };
    // stem: statistics, then the normalised planes and their average
    if (go) AMX_W(launch_pack_tokstem(param(0), sc + P.f_stem_w, sc + P.f_stem_w + 2048, st));
    AMX_W(named("pack_tokstem", hipSuccess));
    TokStemParams sp{};
    sp.x = x; sp.N = n; sp.D = P.D[0]; sp.H = P.H[0]; sp.W = P.W[0];
    sp.w_hi = sc + P.f_stem_w; sp.w_lo = sc + P.f_stem_w + 2048; sp.bias = param(1); sp.stats = stats;
    sp.scale = sc0; sp.shift = sh0; sp.slope = kTokSlope;
    sp.h_hi = sv + P.h_hi[0]; sp.h_lo = sv + P.h_lo[0]; sp.p_hi = sv + P.p_hi[0]; sp.p_lo = sv + P.p_lo[0];
    for (int pass = 0; pass < 2; ++pass) {
      if (go) AMX_W(note(launch_tokstem(sp, pass, st, &li)));
      else { li.report("tokstem<%d,split>", pass); AMX_W(note(hipSuccess)); }
      if (pass == 0)
        AMX_W(finalize(stats, tokstem_slots(P.D[0], P.H[0], P.W[0]), 32, P.vox[0], param(2), param(3), eps, sc0, sh0, (float*)(sv + P.mr[0])));
    }
    for (int k = 0; k < 3; ++k) {
      const int cin = kTokC[k], cout = kTokC[k + 1], b = 4 + S_COUNT * k;
      const size_t b1 = (size_t)(cout / 16) * 27 * (cin / 32) * 1024, b2 = (size_t)(cout / 16) * 27 * (cout / 32) * 1024, bs = (size_t)(cout / 16) * (cin / 32) * 1024;
      if (go) {
        AMX_W(launch_pack_tokconv(param(b + S_C1W), cout, cin, 27, sc + P.f_c1[k], sc + P.f_c1[k] + b1, st));
        AMX_W(launch_pack_tokconv(param(b + S_C2W), cout, cout, 27, sc + P.f_c2[k], sc + P.f_c2[k] + b2, st));
        AMX_W(launch_pack_tokconv(param(b + S_SKW), cout, cin, 1, sc + P.f_sk[k], sc + P.f_sk[k] + bs, st));
      }
      AMX_W(named("pack_tokconv", hipSuccess));
      float *raw1 = (float*)(sv + P.raw1[k]), *raw2 = (float*)(sv + P.raw2[k]), *raws = (float*)(sv + P.raws[k]);
      const long long vo = P.vox[k + 1];
      const TokConvParams c1 = conv_params(sv + P.h_hi[k], sv + P.h_lo[k], k, cin, 2, cout, sc + P.f_c1[k], b1, param(b + S_C1B), raw1, stats);
      AMX_W(conv(c1, 27, 2));
      AMX_W(finalize(stats, tokconv_slots(c1), cout, vo, param(b + S_N1W), param(b + S_N1B), eps, sc0, sh0, (float*)(sv + P.mr[1 + 3 * k])));
      if (go) AMX_W(launch_tok_apply(raw1, n, vo, cout, sc0, sh0, kTokSlope, sv + P.a1_hi[k], sv + P.a1_lo[k], st));
      AMX_W(named("tok_apply", hipSuccess));
      const TokConvParams c2 = conv_params(sv + P.a1_hi[k], sv + P.a1_lo[k], k + 1, cout, 1, cout, sc + P.f_c2[k], b2, param(b + S_C2B), raw2, stats);
      AMX_W(conv(c2, 27, 1));
      AMX_W(finalize(stats, tokconv_slots(c2), cout, vo, param(b + S_N2W), param(b + S_N2B), eps, sc1, sh1, (float*)(sv + P.mr[2 + 3 * k])));
      const TokConvParams sk = conv_params(sv + P.p_hi[k], sv + P.p_lo[k], k + 1, cin, 1, cout, sc + P.f_sk[k], bs, nullptr, raws, stats);
      AMX_W(conv(sk, 1, 1));
      AMX_W(finalize(stats, tokconv_slots(sk), cout, vo, param(b + S_SNW), param(b + S_SNB), eps, sc2, sh2, (float*)(sv + P.mr[3 + 3 * k])));
      if (go)
        AMX_W(launch_tok_combine(raw2, raws, n, P.D[k + 1], P.H[k + 1], P.W[k + 1], cout, sc1, sh1, sc2, sh2, kTokSlope, sv + P.h_hi[k + 1], sv + P.h_lo[k + 1],
                                 k < 2 ? sv + P.p_hi[k + 1] : nullptr, k < 2 ? sv + P.p_lo[k + 1] : nullptr, st));
      AMX_W(named("tok_combine", hipSuccess));
    }
    return exported(sv + P.h_hi[3], sv + P.h_lo[3], 3, 128, out_h3);
  }

  // ---- backward
  // the adjoint of one (rawb null) or two norms behind the activation whose planes are m_hi / m_lo: d_gamma / d_beta, d_raw fp32 into
  // b_fa (, b_fb), their powers of two into cell_a (, cell_b), their planes into b_pa (, b_pb)
  hipError_t norm_adjoint(NadjParams q, int level, const float* gamma_a, const float* gamma_b, float* dga, float* dba, float* dgb, float* dbb, char* sc,
                          float* cell_a, float* cell_b) {
    hipError_t e;
    q.N = P.n; q.vox = P.vox[level]; q.nblk = cdiv(q.vox, kNadjVox);
    q.part = (float*)(sc + P.b_part);
    q.coefa = (const float4*)(sc + P.b_coefa); q.coefb = q.rawb ? (const float4*)(sc + P.b_coefb) : nullptr;
    q.outa = (float*)(sc + P.b_fa); q.outb = (float*)(sc + P.b_fb); q.amax = (float*)(sc + P.b_amax);
    const dim3 grid(q.nblk, P.n);
    if (go) hipLaunchKernelGGL(tok_nadj_kernel<false>, grid, dim3(256), 0, st, q);
    AMX_W(named("tok_nadj_stats", last()));
    if (go)
      hipLaunchKernelGGL(tok_nadj_finalize_kernel, dim3(q.C), dim3(256), 0, st, (const float*)q.part, P.n, q.nblk, q.C, 1.0 / (double)q.vox, gamma_a, q.mra,
                         gamma_b, q.mrb, (float4*)(sc + P.b_coefa), q.rawb ? (float4*)(sc + P.b_coefb) : nullptr, dga, dba, dgb, dbb);
    AMX_W(named("tok_nadj_finalize", last()));
    if (go) hipLaunchKernelGGL(tok_nadj_kernel<true>, grid, dim3(256), 0, st, q);
    AMX_W(named("tok_nadj_apply", last()));
    if (go) hipLaunchKernelGGL(tok_amax_fix_kernel, dim3(q.rawb ? 2 : 1), dim3(256), 0, st, (const float*)q.amax, P.n * q.nblk, cell_a, cell_b);
    AMX_W(named("tok_amax_fix", last()));
    const long long total = (long long)P.n * q.vox * q.C / 8;
    const dim3 sg((unsigned)((total + 255) / 256));
    if (go) hipLaunchKernelGGL(tok_split_kernel, sg, dim3(256), 0, st, (const float*)q.outa, (const float*)cell_a, total, sc + P.b_pa_hi, sc + P.b_pa_lo);
    AMX_W(named("tok_split", last()));
    if (q.rawb) {
      if (go) hipLaunchKernelGGL(tok_split_kernel, sg, dim3(256), 0, st, (const float*)q.outb, (const float*)cell_b, total, sc + P.b_pb_hi, sc + P.b_pb_lo);
      AMX_W(named("tok_split", last()));
    }
    return hipSuccess;
  }
  // dW of the conv (taps, stride) whose output-side planes are d_hi / d_lo (level lvl_out, Cout) and whose input planes are x_hi / x_lo
  hipError_t wgrad(const char* d_hi, const char* d_lo, int lvl_out, int Cout, const char* x_hi, const char* x_lo, int lvl_in, int Cin, int taps, int stride,
                   const float* cell, float* dw, char* sc) {
    hipError_t e;
    TokWgradParams w{};
    w.d_hi = d_hi; w.d_lo = d_lo; w.N = P.n; w.Do = P.D[lvl_out]; w.Ho = P.H[lvl_out]; w.Wo = P.W[lvl_out]; w.Cout = Cout;
    w.x_hi = x_hi; w.x_lo = x_lo; w.D = P.D[lvl_in]; w.H = P.H[lvl_in]; w.W = P.W[lvl_in]; w.Cin = Cin;
    w.steps = (int)((long long)P.n * P.vox[lvl_out] / 32);
    w.chunks = wgrad_chunks((long long)P.n * P.vox[lvl_out], &w.spc);
    w.part = (float*)(sc + P.b_wpart);
    const dim3 grid(cdiv(w.chunks, 4), (Cout / 32) * (Cin / 32), taps);
    if (go) {
      if (taps == 27 && stride == 2) hipLaunchKernelGGL((tokwgrad_kernel<27, 2>), grid, dim3(256), 0, st, w);
      else if (taps == 27) hipLaunchKernelGGL((tokwgrad_kernel<27, 1>), grid, dim3(256), 0, st, w);
      else hipLaunchKernelGGL((tokwgrad_kernel<1, 1>), grid, dim3(256), 0, st, w);
    }
    li.report("tokwgrad<%d,%d>", taps, stride);
    AMX_W(note(last()));
    const long long count = (long long)Cout * Cin * taps;
    if (go) hipLaunchKernelGGL(tok_wgrad_reduce_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const float*)w.part, w.chunks, count, cell, dw);
    return named("tok_wgrad_reduce", last());
  }
  hipError_t pack_t(const float* w, int Cout, int Cin, int taps, int flip, char* dst, size_t plane) {
    const long long cnt = (long long)(Cin / 16) * taps * (Cout / 32) * 64;
    if (go) hipLaunchKernelGGL(tok_pack_t_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, w, Cout, Cin, taps, flip, (f16*)dst, (f16*)(dst + plane));
    return named("tok_pack_t", last());
  }
  hipError_t zero(float* dst, int count) {
    if (!dst) return hipSuccess;
    return named("zero", go ? hipMemsetAsync(dst, 0, (size_t)count * 4, st) : hipSuccess);
  }

  hipError_t backward(const float* d_h3, const float* x, const float* const* prm, const char* sv, float* const* grads, char* sc) {
    hipError_t e;
    const int n = P.n;
    auto param = [&](int i) { return go ? prm[i] : (const float*)nullptr; };
    static float every;                                                      // the report walk states every output (never written)
    auto grad = [&](int i) { return go ? grads[i] : &every; };
    auto cell = [&](int i) { return (float*)(sc + P.b_cell + 256 * i); };
    char *pa_hi = sc + P.b_pa_hi, *pa_lo = sc + P.b_pa_lo, *pb_hi = sc + P.b_pb_hi, *pb_lo = sc + P.b_pb_lo;
    float *fb = (float*)(sc + P.b_fb), *dpool = (float*)(sc + P.b_dpool);
    for (int k = 2; k >= 0; --k) {
      const int cin = kTokC[k], cout = kTokC[k + 1], b = 4 + S_COUNT * k, lo = k + 1;
      float *cell2 = cell(3 * k), *cells = cell(3 * k + 1), *cell1 = cell(3 * k + 2);
      const size_t wplane_c = (size_t)(cout / 16) * 27 * (cout / 32) * 1024, wplane_1 = (size_t)(cin / 16) * 27 * (cout / 32) * 1024;
      const size_t wplane_s = (size_t)(cin / 16) * (cout / 32) * 1024;
      // norm2 and skip_norm behind the stage's closing LeakyReLU
      NadjParams q{};
      if (k == 2) { q.d = d_h3; q.sn = (long long)cout * P.vox[3]; q.sv = 1; q.sc = P.vox[3]; }          // NCDHW from autograd
      else { q.d = (const float*)(sc + P.b_dh[k + 1]); q.sn = (long long)cout * P.vox[lo]; q.sv = cout; q.sc = 1; }
      q.m_hi = sv + P.h_hi[lo]; q.m_lo = sv + P.h_lo[lo]; q.C = cout;
      q.rawa = (const float*)(sv + P.raw2[k]); q.rawb = (const float*)(sv + P.raws[k]);
      q.mra = (const float*)(sv + P.mr[2 + 3 * k]); q.mrb = (const float*)(sv + P.mr[3 + 3 * k]);
      AMX_W(norm_adjoint(q, lo, param(b + S_N2W), param(b + S_SNW), grad(b + S_N2W), grad(b + S_N2B), grad(b + S_SNW), grad(b + S_SNB), sc, cell2, cells));
      // skip branch: 1x1x1 weight gradient; data gradient -> gradient of the pooled stage input
      if (grad(b + S_SKW)) AMX_W(wgrad(pb_hi, pb_lo, lo, cout, sv + P.p_hi[k], sv + P.p_lo[k], lo, cin, 1, 1, cells, grad(b + S_SKW), sc));
      AMX_W(pack_t(param(b + S_SKW), cout, cin, 1, 0, sc + P.b_wt, wplane_s));
      AMX_W(conv(conv_params(pb_hi, pb_lo, lo, cout, 1, cin, sc + P.b_wt, wplane_s, nullptr, dpool, nullptr), 1, 1));
      // conv2: weight gradient; stride-1 data gradient (flipped, transposed weights) -> gradient of a1, times 2^-e2
      if (grad(b + S_C2W)) AMX_W(wgrad(pa_hi, pa_lo, lo, cout, sv + P.a1_hi[k], sv + P.a1_lo[k], lo, cout, 27, 1, cell2, grad(b + S_C2W), sc));
      AMX_W(zero(grad(b + S_C2B), cout));
      AMX_W(pack_t(param(b + S_C2W), cout, cout, 27, 1, sc + P.b_wt, wplane_c));
      AMX_W(conv(conv_params(pa_hi, pa_lo, lo, cout, 1, cout, sc + P.b_wt, wplane_c, nullptr, fb, nullptr), 27, 1));
      // norm1 behind the inner LeakyReLU
      NadjParams q1{};
      q1.d = fb; q1.sn = (long long)cout * P.vox[lo]; q1.sv = cout; q1.sc = 1; q1.dscale = cell2 + 1;
      q1.m_hi = sv + P.a1_hi[k]; q1.m_lo = sv + P.a1_lo[k]; q1.C = cout;
      q1.rawa = (const float*)(sv + P.raw1[k]); q1.mra = (const float*)(sv + P.mr[1 + 3 * k]);
      AMX_W(norm_adjoint(q1, lo, param(b + S_N1W), nullptr, grad(b + S_N1W), grad(b + S_N1B), nullptr, nullptr, sc, cell1, nullptr));
      // conv1: weight gradient; stride-2 data gradient + the AvgPool adjoint -> gradient of the stage input
      if (grad(b + S_C1W)) AMX_W(wgrad(pa_hi, pa_lo, lo, cout, sv + P.h_hi[k], sv + P.h_lo[k], k, cin, 27, 2, cell1, grad(b + S_C1W), sc));
      AMX_W(zero(grad(b + S_C1B), cout));
      AMX_W(pack_t(param(b + S_C1W), cout, cin, 27, 0, sc + P.b_wt, wplane_1));
      TokDgrad2Params dg{};
      dg.d_hi = pa_hi; dg.d_lo = pa_lo; dg.N = n; dg.Do = P.D[lo]; dg.Ho = P.H[lo]; dg.Wo = P.W[lo]; dg.Cout = cout; dg.Cin = cin;
      dg.w_hi = sc + P.b_wt; dg.w_lo = sc + P.b_wt + wplane_1; dg.scale = cell1 + 1; dg.dpool = dpool; dg.pscale = cells + 1;
      dg.out = (float*)(sc + P.b_dh[k]);
      const long long waves = (long long)n * P.vox[lo] / 32;
      if (go) hipLaunchKernelGGL((tokdgrad2_kernel<2, 2>), dim3((unsigned)((waves + 3) / 4), cin / 32, 8), dim3(256), 0, st, dg);
      li.report("tokdgrad2<2,2>");
      AMX_W(note(last()));
    }
    // stem
    TokStemBwdParams sp{};
    sp.x = x; sp.N = n; sp.D = P.D[0]; sp.H = P.H[0]; sp.W = P.W[0]; sp.nblk = cdiv(P.vox[0], kStemVox);
    sp.w = param(0); sp.bias = param(1); sp.mr = (const float*)(sv + P.mr[0]); sp.dh = (const float*)(sc + P.b_dh[0]);
    sp.m_hi = sv + P.h_hi[0]; sp.m_lo = sv + P.h_lo[0];
    sp.part = (float*)(sc + P.b_part); sp.coef = (const float4*)(sc + P.b_coefa); sp.wpart = (float*)(sc + P.b_wpart);
    const dim3 grid(sp.nblk, n);
    if (go) hipLaunchKernelGGL(tokstem_bwd_kernel<0>, grid, dim3(256), 0, st, sp);
    li.report("tokstem_bwd<0>");
    AMX_W(note(last()));
    if (go)
      hipLaunchKernelGGL(tok_nadj_finalize_kernel, dim3(32), dim3(256), 0, st, (const float*)sp.part, n, sp.nblk, 32, 1.0 / (double)P.vox[0], param(2), sp.mr,
                         (const float*)nullptr, (const float*)nullptr, (float4*)(sc + P.b_coefa), (float4*)nullptr, grad(2), grad(3), (float*)nullptr,
                         (float*)nullptr);
    AMX_W(named("tok_nadj_finalize", last()));
    if (grad(0)) {
      if (go) hipLaunchKernelGGL(tokstem_bwd_kernel<1>, grid, dim3(256), 0, st, sp);
      li.report("tokstem_bwd<1>");
      AMX_W(note(last()));
      if (go)
        hipLaunchKernelGGL(tok_wgrad_reduce_kernel, dim3((32 * 27 + 255) / 256), dim3(256), 0, st, (const float*)sp.wpart, n * sp.nblk, (long long)32 * 27,
                           (const float*)nullptr, grad(0));
      AMX_W(named("tok_wgrad_reduce", last()));
    }
    return zero(grad(1), 32);
#undef AMX_W
  }
};

bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return !(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15);
}

int plan_or_refuse(const char* what, int n, int D, int H, int W, TrainPlan* P) {
  if (!train_plan(n, D, H, W, P))
    return fail(AMX_ERR_SHAPE,
                "%s: n = %d, %d x %d x %d is outside the envelope (W a multiple of 16, D and H of 8, a multiple of 64 tokens, at most 2^22 voxels in all)", what, n,
                D, H, W);
  return AMX_OK;
}

}  // namespace
}  // namespace amx

extern "C" {

size_t amx_tokenizer_train_saved_bytes(int n, int D, int H, int W) {
  amx::TrainPlan P;
  return amx::train_plan(n, D, H, W, &P) ? P.saved_bytes : 0;
}

size_t amx_tokenizer_train_scratch_bytes(int n, int D, int H, int W) {
  amx::TrainPlan P;
  return amx::train_plan(n, D, H, W, &P) ? (P.fwd_bytes > P.bwd_bytes ? P.fwd_bytes : P.bwd_bytes) : 0;
}

int amx_tokenizer_train_forward(const float* d_x, const float* const* params, int n, int D, int H, int W, float in_eps, float* d_h3, void* d_saved,
                                size_t saved_bytes, void* d_scratch, size_t scratch_bytes, void* stream) {
  using namespace amx;
  TrainPlan P;
  if (int rc = plan_or_refuse("tokenizer train forward", n, D, H, W, &P)) return rc;
  if (!d_x || !params || !d_h3) return fail(AMX_ERR_INVALID, "tokenizer train forward: null argument");
  for (int i = 0; i < kTokParams; ++i)
    if (!params[i] || !aligned16(params[i])) return fail(AMX_ERR_INVALID, "tokenizer train forward: parameter %d is null or not 16-byte aligned", i);
  if (!d_saved || saved_bytes < P.saved_bytes || !aligned16(d_saved)) return fail(AMX_ERR_WORKSPACE, "tokenizer saved state needs %zu bytes, 16-byte aligned", P.saved_bytes);
  if (!d_scratch || scratch_bytes < P.fwd_bytes || !aligned16(d_scratch)) return fail(AMX_ERR_WORKSPACE, "tokenizer train scratch needs %zu bytes, 16-byte aligned", P.fwd_bytes);
  if (!aligned16(d_x, d_h3)) return fail(AMX_ERR_INVALID, "tokenizer train forward: d_x and d_h3 must be 16-byte aligned");
  Walk w{P, (hipStream_t)stream, true, nullptr};
  AMX_HIP(w.forward(d_x, params, in_eps, d_h3, (char*)d_saved, (char*)d_scratch));
  return AMX_OK;
}

int amx_tokenizer_backward(const float* d_dh3, const float* d_x, const float* const* params, const void* d_saved, int n, int D, int H, int W, float in_eps,
                           float* const* grads, void* d_scratch, size_t scratch_bytes, void* stream) {
  using namespace amx;
  (void)in_eps;                       // the saved rstd already holds it
  TrainPlan P;
  if (int rc = plan_or_refuse("tokenizer backward", n, D, H, W, &P)) return rc;
  if (!d_dh3 || !d_x || !params || !d_saved || !grads) return fail(AMX_ERR_INVALID, "tokenizer backward: null argument");
  for (int i = 0; i < kTokParams; ++i) {
    if (!params[i] || !aligned16(params[i])) return fail(AMX_ERR_INVALID, "tokenizer backward: parameter %d is null or not 16-byte aligned", i);
    if (grads[i] && !aligned16(grads[i])) return fail(AMX_ERR_INVALID, "tokenizer backward: gradient %d is not 16-byte aligned", i);
  }
  if (!d_scratch || scratch_bytes < P.bwd_bytes || !aligned16(d_scratch)) return fail(AMX_ERR_WORKSPACE, "tokenizer train scratch needs %zu bytes, 16-byte aligned", P.bwd_bytes);
  if (!aligned16(d_dh3, d_x, d_saved)) return fail(AMX_ERR_INVALID, "tokenizer backward: d_dh3, d_x and d_saved must be 16-byte aligned");
  Walk w{P, (hipStream_t)stream, true, nullptr};
  AMX_HIP(w.backward(d_dh3, d_x, params, (const char*)d_saved, grads, (char*)d_scratch));
  return AMX_OK;
}

int amx_tokenizer_train_export(const void* d_saved, int n, int D, int H, int W, int site, float* d_out) {
  using namespace amx;
  TrainPlan P;
  if (int rc = plan_or_refuse("tokenizer train export", n, D, H, W, &P)) return rc;
  if (!d_saved || !d_out) return fail(AMX_ERR_INVALID, "tokenizer train export: null argument");
  if (site < 0 || site > 6) return fail(AMX_ERR_INVALID, "tokenizer train export: site 0 .. 6 (h0, a1 of stage 0, h1, a1 of stage 1, h2, a1 of stage 2, h3), got %d", site);
  const char* sv = (const char*)d_saved;
  const int k = site / 2;
  AMX_HIP(hipDeviceSynchronize());
  Walk w{P, nullptr, true, nullptr};
  if (site & 1) AMX_HIP(w.exported(sv + P.a1_hi[k], sv + P.a1_lo[k], k + 1, kTokC[k + 1], d_out));
  else AMX_HIP(w.exported(sv + P.h_hi[k], sv + P.h_lo[k], k, kTokC[k], d_out));
  AMX_HIP(hipDeviceSynchronize());
  return AMX_OK;
}

int amx_tokenizer_train_route(int n, int D, int H, int W, char* buf, size_t cap) {
  using namespace amx;
  TrainPlan P;
  if (int rc = plan_or_refuse("tokenizer train route", n, D, H, W, &P)) return rc;
  if (!buf || cap < 1) return fail(AMX_ERR_INVALID, "tokenizer train route: null buffer");
  std::string log;
  Walk w{P, nullptr, false, &log};
  (void)w.forward(nullptr, nullptr, 0.f, nullptr, nullptr, nullptr);
  (void)w.backward(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (log.size() + 1 > cap) return fail(AMX_ERR_WORKSPACE, "tokenizer train route: the report needs %zu bytes", log.size() + 1);
  memcpy(buf, log.c_str(), log.size() + 1);
  return AMX_OK;
}

}  // extern "C"
