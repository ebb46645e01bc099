// anatomix_amd -- backward of the fused attention core (amx_attention.hip): gradients of
//   out = softmax(rope(q_norm(q)) rope(k_norm(k))^T / sqrt(hd)) v
// with respect to q, k, v and the affine parameters of the two per-head LayerNorms, flash-style: the N x N probabilities are
// recomputed from the forward's f16 operands and its saved log-sum-exp, never stored.  With q^, k^, v^ the prepared f16 operands
// (q^ carries log2(e) / sqrt(hd)) and everything in the exp2 domain:
//   P = exp2(S - lse), S = q^ k^T      D_i = sum_d dO_id O_id      dP = dO^ v^T      dS = P o (dP - D)
//   dV = P^T dO^      dq^ = ln2 dS k^      dk^ = ln2 dS^T q^
// then the adjoint of the preparation (rotation transposed on the patch tokens, LayerNorm backward from the saved fp32 q / k).
//
// Passes (launch_attention_backward):
//   attn_prep<TRAIN>   re-runs the forward's preparation: no operand buffer is kept per layer.  Besides the forward's images it writes
//                      V as a ROW image and K^, Q^ as COL images (amx_attention.h).
//   attn_delta         D in fp32 from the UNROUNDED dO and O; max |dO| per 64-token block.
//   attn_dprep         one power of two per (batch, head) from those maxima, 2^e <= max |dO| / 8 < 2^(e+1): dO^ = f16(dO 2^-e) as rows and
//                      as a COL image, D 2^-e, the log-sum-exp padded (padding rows: huge, so their P is 0).  No host read-back; the
//                      epilogues multiply by 2^e.  An all-zero dO takes e = 0 and gives exact zeros.
//   attn_bwd_dkv       a block of 128 KEYS stationary (K^ and V^ ROW fragments resident in registers), the query blocks stream past:
//                      S = Q^ K^T and dP = dO^ V^T leave the MFMA with a lane owning ONE key, so P and dS in accumulator layout are
//                      already the B operands of dV^T += dO^T P and dK^T += Q^T dS (A operands: the COL images).
//   attn_bwd_dq        the forward's own transposed layout, 128 QUERIES stationary, the key blocks stream past: S^T = K^ Q^T,
//                      dP^T = V^ dO^T, a lane owns ONE query and dS^T in registers is the B operand of dQ^T += K^T dS^T.
//   attn_prep_bwd      rotation^T, LayerNorm backward; per-block sums of the norm gradients, added by attn_norm_reduce in a fixed order.
// P is recomputed in both main kernels (7 matrix products against 5): every output element then has one owner -- no atomics, one
// summation order, bit-identical results run to run.  -lse and -D are the INITIAL accumulators of the S and dP chains.
// Both main kernels stage their stream through two LDS buffers filled by LDS-DMA, one `s_waitcnt vmcnt(0)` + `__syncthreads()` per
// block (the forward's barrier-free loader handshake is not used here).  v_mfma_f32_16x16x32_f16, fp32 accumulation; softmax and
// dP - D in fp32; roundings to f16: q^, k^, v^ (the forward's), dO^ (scaled), P and dS.
#include <math.h>
#include <stdio.h>

#include <type_traits>

#include "amx_attention.h"
#include "amx_device.h"
#include "amx_launch.h"

namespace amx {

constexpr int kAttGradExp = 3;        // max |dO^| of a (batch, head) lies in [2^3, 2^4)
constexpr float kAttLsePad = 3.0e38f; // log-sum-exp of a padding row: exp2(S - this) = 0
constexpr int kAttRowB = kAttKRow * 2;            // bytes per Qp / dOp row
constexpr int kAttRowsPieces = kAttBN * kAttRowB / 1024;   // 1 KiB pieces of 64 rows
static_assert(kAttRowsPieces * 1024 == kAttBN * kAttRowB, "64 operand rows are whole 1 KiB pieces");

namespace {

// wave-wide sum on the VALU (attn_prep's: DPP row shifts + row broadcasts, total read from lane 63); a fixed order
__device__ __forceinline__ float att_wave_sum(float x) {
  auto dpp = [](float v, auto CTRL, auto ROWS) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(CTRL)::value, decltype(ROWS)::value, 0xF, true));
  };
  x += dpp(x, std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xF>{});
  x += dpp(x, std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xF>{});
  x += dpp(x, std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xF>{});
  x += dpp(x, std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xF>{});
  x += dpp(x, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xA>{});
  x += dpp(x, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xC>{});
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}

// grid (ceil(n / 64), heads, b), block 256 = 4 waves x 16 tokens, lane d holds channels d and d + 64
__global__ __launch_bounds__(256) void attn_delta_kernel(const float* __restrict__ dout, const float* __restrict__ out, int n, int heads,
                                                         int hd, float* __restrict__ Draw, float* __restrict__ amax) {
  __shared__ float wmax[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.y, b = blockIdx.z, npad = att_npad(n);
  const long long bh = (long long)b * heads + h;
  const bool a0 = lane < hd, a1 = lane + 64 < hd;
  float am = 0.f;
  for (int i = 0; i < 16; ++i) {
    const int tok = blockIdx.x * kAttBN + wave * 16 + i;
    if (tok >= n) break;
    const long long src = ((long long)b * n + tok) * heads * hd + (long long)h * hd;
    const float g0 = a0 ? dout[src + lane] : 0.f, g1 = a1 ? dout[src + lane + 64] : 0.f;
    const float o0 = a0 ? out[src + lane] : 0.f, o1 = a1 ? out[src + lane + 64] : 0.f;
    const float d = att_wave_sum(g0 * o0 + g1 * o1);
    am = fmaxf(am, fmaxf(fabsf(g0), fabsf(g1)));
    if (lane == 0) Draw[bh * npad + tok] = d;
  }
  for (int o = 32; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 64));
  if (lane == 0) wmax[wave] = am;
  __syncthreads();
  if (threadIdx.x == 0) amax[bh * (npad / kAttBN) + blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

// grid (n_pad / 64, heads, b), block 256
__global__ __launch_bounds__(256) void attn_dprep_kernel(const float* __restrict__ dout, const float* __restrict__ lse,
                                                         const float* __restrict__ Draw, const float* __restrict__ amax, int n, int heads,
                                                         int hd, f16* __restrict__ dOp, f16* __restrict__ dOt, float* __restrict__ lsep,
                                                         float* __restrict__ Dp, float* __restrict__ scl) {
  __shared__ __attribute__((aligned(16))) f16 dcol[kAttVFrag * 512];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.y, b = blockIdx.z, npad = att_npad(n), nblk = (n + kAttBN - 1) / kAttBN, nblk_pad = npad / kAttBN;
  const long long bh = (long long)b * heads + h;
  for (int i = threadIdx.x; i < kAttVFrag * 64; i += 256) ((uint4*)dcol)[i] = make_uint4(0u, 0u, 0u, 0u);
  // the (batch, head)'s power of two: every workgroup of the pair derives the same one from the same maxima
  float am = 0.f;
  for (int i = 0; i < nblk; ++i) am = fmaxf(am, amax[bh * nblk_pad + i]);
  const unsigned bits = __builtin_bit_cast(unsigned, am);
  const int field = (int)((bits >> 23) & 0xffu);
  int e = 0;
  if (am > 0.f && field != 255) {
    e = field - 127 - kAttGradExp;
    e = e < -126 ? -126 : (e > 126 ? 126 : e);
  }
  const float sdown = __builtin_bit_cast(float, (unsigned)(127 - e) << 23), sup = __builtin_bit_cast(float, (unsigned)(127 + e) << 23);
  if (blockIdx.x == 0 && threadIdx.x == 0) { scl[bh * 2] = sdown; scl[bh * 2 + 1] = sup; }
  __syncthreads();
  const bool a0 = lane < hd, a1 = lane + 64 < hd;
  for (int i = 0; i < 16; ++i) {
    const int tib = wave * 16 + i, tok = blockIdx.x * kAttBN + tib;
    const long long row = bh * npad + tok;
    f16* dro = dOp + row * kAttKRow;
    if (tok >= n) {
      for (int d = lane; d < kAttKRow; d += 64) dro[d] = (f16)0.f;
      if (lane == 0) { lsep[row] = kAttLsePad; Dp[row] = 0.f; }
      continue;
    }
    const long long src = ((long long)b * n + tok) * heads * hd + (long long)h * hd;
    const float g0 = a0 ? dout[src + lane] * sdown : 0.f, g1 = a1 ? dout[src + lane + 64] * sdown : 0.f;
    dro[lane] = (f16)g0;
    if (lane + 64 < kAttKRow) dro[lane + 64] = (f16)g1;
    if (a0) dcol[att_col_idx(tib, lane)] = (f16)g0;
    if (a1) dcol[att_col_idx(tib, lane + 64)] = (f16)g1;
    if (lane == 0) { lsep[row] = lse[bh * n + tok]; Dp[row] = Draw[row] * sdown; }
  }
  __syncthreads();
  uint4* dd = (uint4*)(dOt + (bh * nblk_pad + blockIdx.x) * (kAttVFrag * 512));
  for (int i = threadIdx.x; i < kAttVFrag * 64; i += 256) dd[i] = ((const uint4*)dcol)[i];
}

// one 1 KiB piece (16 bytes per lane) global -> LDS
__device__ __forceinline__ void att_piece(const char* src, unsigned lds_base, int j, int lane) {
  dma16_asm(src + lane * 16, (unsigned)__builtin_amdgcn_readfirstlane((int)(lds_base + (unsigned)j * 1024u)));
}

// grid (n_pad / 128, heads, b), block 256 = 4 waves x 32 keys (2 key tiles of 16).  Dynamic LDS: 2 buffers of
// {Q^ rows | dO^ rows | Q^T COL image | dO^T COL image} of one 64-query block.
constexpr int kDkvRows = kAttBN * kAttRowB, kDkvCol = kAttVFrag * 1024, kDkvBuf = 2 * kDkvRows + 2 * kDkvCol;
constexpr int kDkvLds = 2 * kDkvBuf;
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const f16* __restrict__ Qp, const f16* __restrict__ Kp, const f16* __restrict__ Vr,
                                                           const f16* __restrict__ Qt, const f16* __restrict__ dOp, const f16* __restrict__ dOt,
                                                           const float* __restrict__ lsep, const float* __restrict__ Dp,
                                                           const float* __restrict__ scl, int n, int heads, int hd,
                                                           float* __restrict__ dkh, float* __restrict__ dv) {
  constexpr int KT = 2, NP = kDkvBuf / 1024, PR = kAttRowsPieces, PC = kAttVFrag;
  static_assert(NP == 2 * PR + 2 * PC, "pieces per block");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, npad = att_npad(n);
  const long long bh = (long long)b * heads + h;
  const int nblk = (n + kAttBN - 1) / kAttBN, nblk_pad = npad / kAttBN;
  const unsigned lds0 = lds_addr(smem);
  const char* qrows = (const char*)(Qp + bh * npad * kAttKRow);
  const char* drows = (const char*)(dOp + bh * npad * kAttKRow);
  const char* qcols = (const char*)(Qt + bh * nblk_pad * (kAttVFrag * 512));
  const char* dcols = (const char*)(dOt + bh * nblk_pad * (kAttVFrag * 512));
  auto issue = [&](int blk, int bsel) {
    const unsigned base = lds0 + (unsigned)bsel * kDkvBuf;
#pragma unroll
    for (int r = 0; r < (NP + 3) / 4; ++r) {
      const int j = wave + 4 * r;                          // wave-uniform
      if (j < PR) att_piece(qrows + (long long)blk * kDkvRows + j * 1024, base, j, lane);
      else if (j < 2 * PR) att_piece(drows + (long long)blk * kDkvRows + (j - PR) * 1024, base, j, lane);
      else if (j < 2 * PR + PC) att_piece(qcols + (long long)blk * kDkvCol + (j - 2 * PR) * 1024, base, j, lane);
      else if (j < NP) att_piece(dcols + (long long)blk * kDkvCol + (j - 2 * PR - PC) * 1024, base, j, lane);
    }
  };
  issue(0, 0);

  // resident B fragments: lane (i, g) holds K^[key i][32 kk + 8 g .. + 7] (and V^ likewise) of its two key tiles
  const int tile0 = blockIdx.x * 8 + wave * KT;            // 16-key tile index within the (batch, head)
  f16x8 kf[KT][3], vf[KT][3];
  bool kvalid[KT];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
    const int tile = tile0 + kt;
    const long long frag = (bh * nblk_pad + (tile >> 2)) * kAttKFrag + (tile & 3) * 3;
    kvalid[kt] = tile * 16 + li < n;
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) {
      kf[kt][kk] = *(const f16x8*)(Kp + ((frag + kk) * 64 + lane) * 8);
      vf[kt][kk] = *(const f16x8*)(Vr + ((frag + kk) * 64 + lane) * 8);
    }
  }
  f32x4 acc_dv[KT][5], acc_dk[KT][5];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
#pragma unroll
    for (int dt = 0; dt < 5; ++dt) acc_dv[kt][dt] = acc_dk[kt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // -lse and -D of the lane's 16 queries of a block (4 g .. 4 g + 3 of each tile), fetched one block ahead and BEFORE that block's
  // DMA is issued: the compiler's wait for them then falls behind the loop's own vmcnt(0) instead of draining the prefetch early
  f32x4 nl4[4], nd4[4], nl4_next[4], nd4_next[4];
  auto fetch_rows = [&](int blk, f32x4* l, f32x4* d) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const long long r = bh * npad + blk * kAttBN + t * 16 + 4 * g;
      l[t] = -*(const f32x4*)(lsep + r);
      d[t] = -*(const f32x4*)(Dp + r);
    }
  };
  fetch_rows(0, nl4, nd4);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int blk = 0; blk < nblk; ++blk) {
    if (blk + 1 < nblk) {
      fetch_rows(blk + 1, nl4_next, nd4_next);
      issue(blk + 1, (blk + 1) & 1);
    }
    const char* sQ = smem + (blk & 1) * kDkvBuf;
    const char* sD = sQ + kDkvRows;
    const char* sQt = sD + kDkvRows;
    const char* sDt = sQt + kDkvCol;
    // ---- S - lse and dP - D: lane (i, g) holds queries 16 t + 4 g + j of key i
    f32x4 acc_s[4][KT], acc_p[4][KT];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) { acc_s[t][kt] = nl4[t]; acc_p[t][kt] = nd4[t]; }
#pragma unroll
    for (int kk = 0; kk < 3; ++kk)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f16x8 qa = *(const f16x8*)(sQ + (t * 16 + li) * kAttRowB + kk * 64 + g * 16);
        const f16x8 da = *(const f16x8*)(sD + (t * 16 + li) * kAttRowB + kk * 64 + g * 16);
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          acc_s[t][kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qa, kf[kt][kk], acc_s[t][kt], 0, 0, 0);
          acc_p[t][kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(da, vf[kt][kk], acc_p[t][kt], 0, 0, 0);
        }
      }
    // ---- P and dS, straight into the B fragments of the two accumulating products (queries of a K step in COL-image order)
    f16x8 pf[KT][2], sf[KT][2];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float pr = kvalid[kt] ? __builtin_amdgcn_exp2f(acc_s[t][kt][j]) : 0.f;
          pf[kt][t >> 1][(t & 1) * 4 + j] = (f16)pr;
          sf[kt][t >> 1][(t & 1) * 4 + j] = (f16)(pr * acc_p[t][kt][j]);
        }
    // ---- dV^T += dO^T P, dK^T += Q^T dS
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int dt = 0; dt < 5; ++dt) {
        const f16x8 da = *(const f16x8*)(sDt + ((dt * 2 + ks) * 64 + lane) * 16);
        const f16x8 qa = *(const f16x8*)(sQt + ((dt * 2 + ks) * 64 + lane) * 16);
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          acc_dv[kt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(da, pf[kt][ks], acc_dv[kt][dt], 0, 0, 0);
          acc_dk[kt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qa, sf[kt][ks], acc_dk[kt][dt], 0, 0, 0);
        }
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the next block has landed; everyone is through with this one
    __syncthreads();
    if (blk + 1 < nblk) {
#pragma unroll
      for (int t = 0; t < 4; ++t) { nl4[t] = nl4_next[t]; nd4[t] = nd4_next[t]; }
    }
  }
  // ---- epilogue: lane (i, g) holds dV^T / dK^T [dim 16 dt + 4 g + j][key i]; undo the power of two
  const float sup = scl[bh * 2 + 1], ksc = 0.6931471805599453f * sup;
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
    const int key = (tile0 + kt) * 16 + li;
    if (key >= n) continue;
    const long long o = ((long long)b * n + key) * heads * hd + (long long)h * hd;
#pragma unroll
    for (int dt = 0; dt < 5; ++dt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = dt * 16 + 4 * g + j;
        if (d < hd) {
          if (dv != nullptr) dv[o + d] = acc_dv[kt][dt][j] * sup;
          dkh[o + d] = acc_dk[kt][dt][j] * ksc;
        }
      }
  }
}

// grid (n_pad / 128, heads, b), block 256 = 4 waves x 32 queries (2 query tiles).  Dynamic LDS: 2 buffers of
// {K^ ROW image | V^ ROW image | K^T COL image} of one 64-key block.
constexpr int kDqRow = kAttKFrag * 1024, kDqCol = kAttVFrag * 1024, kDqBuf = 2 * kDqRow + kDqCol;
constexpr int kDqLds = 2 * kDqBuf;
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const f16* __restrict__ Qp, const f16* __restrict__ Kp, const f16* __restrict__ Vr,
                                                          const f16* __restrict__ Kt, const f16* __restrict__ dOp,
                                                          const float* __restrict__ lsep, const float* __restrict__ Dp,
                                                          const float* __restrict__ scl, int n, int heads, int hd, float* __restrict__ dqh) {
  constexpr int QT = kAttQT, NP = kDqBuf / 1024, PR = kAttKFrag;
  static_assert(NP == 2 * PR + kAttVFrag, "pieces per block");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, npad = att_npad(n);
  const long long bh = (long long)b * heads + h;
  const int nblk = (n + kAttBN - 1) / kAttBN, nblk_pad = npad / kAttBN;
  const unsigned lds0 = lds_addr(smem);
  const char* krow = (const char*)(Kp + bh * nblk_pad * (kAttKFrag * 512));
  const char* vrow = (const char*)(Vr + bh * nblk_pad * (kAttKFrag * 512));
  const char* kcol = (const char*)(Kt + bh * nblk_pad * (kAttVFrag * 512));
  auto issue = [&](int blk, int bsel) {
    const unsigned base = lds0 + (unsigned)bsel * kDqBuf;
#pragma unroll
    for (int r = 0; r < (NP + 3) / 4; ++r) {
      const int j = wave + 4 * r;                          // wave-uniform
      if (j < PR) att_piece(krow + (long long)blk * kDqRow + j * 1024, base, j, lane);
      else if (j < 2 * PR) att_piece(vrow + (long long)blk * kDqRow + (j - PR) * 1024, base, j, lane);
      else if (j < NP) att_piece(kcol + (long long)blk * kDqCol + (j - 2 * PR) * 1024, base, j, lane);
    }
  };
  issue(0, 0);

  const int q0 = blockIdx.x * kAttBM + wave * 16 * QT;
  // resident B fragments: lane (i, g) holds Q^[query q0 + 16 qt + i][32 kk + 8 g .. + 7], dO^ likewise; -lse and -D of that query
  f16x8 qf[QT][3], df[QT][3];
  f32x4 nl[QT], nd[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const long long row = bh * npad + q0 + qt * 16 + li;
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) {
      qf[qt][kk] = *(const f16x8*)(Qp + row * kAttKRow + kk * 32 + g * 8);
      df[qt][kk] = *(const f16x8*)(dOp + row * kAttKRow + kk * 32 + g * 8);
    }
    const float l = -lsep[row], d = -Dp[row];
    nl[qt] = f32x4{l, l, l, l};
    nd[qt] = f32x4{d, d, d, d};
  }
  f32x4 acc_dq[QT][5];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int dt = 0; dt < 5; ++dt) acc_dq[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int blk = 0; blk < nblk; ++blk) {
    if (blk + 1 < nblk) issue(blk + 1, (blk + 1) & 1);
    const char* sK = smem + (blk & 1) * kDqBuf;
    const char* sV = sK + kDqRow;
    const char* sKt = sV + kDqRow;
    // ---- S^T - lse = K^ Q^T, dP^T - D = V^ dO^T: lane (i, g) holds keys 16 kt + 4 g + j of query i
    f32x4 acc_s[QT][4], acc_p[QT][4];
#pragma unroll
    for (int kk = 0; kk < 3; ++kk)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const f16x8 ka = *(const f16x8*)(sK + ((kt * 3 + kk) * 64 + lane) * 16);
        const f16x8 va = *(const f16x8*)(sV + ((kt * 3 + kk) * 64 + lane) * 16);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          acc_s[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ka, qf[qt][kk], kk == 0 ? nl[qt] : acc_s[qt][kt], 0, 0, 0);
          acc_p[qt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, df[qt][kk], kk == 0 ? nd[qt] : acc_p[qt][kt], 0, 0, 0);
        }
      }
    if ((blk + 1) * kAttBN > n) {      // keys beyond the sequence (last block only): P = 0, as the forward masks them
      asm volatile("" ::: "memory");
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (blk * kAttBN + kt * 16 + 4 * g + j >= n) {
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) acc_s[qt][kt][j] = -3.0e38f;
          }
    }
    // ---- dS^T straight into the B fragments of dQ^T += K^T dS^T
    f16x8 sf[QT][2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          sf[qt][kt >> 1][(kt & 1) * 4 + j] = (f16)(__builtin_amdgcn_exp2f(acc_s[qt][kt][j]) * acc_p[qt][kt][j]);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int dt = 0; dt < 5; ++dt) {
        const f16x8 ka = *(const f16x8*)(sKt + ((dt * 2 + ks) * 64 + lane) * 16);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) acc_dq[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ka, sf[qt][ks], acc_dq[qt][dt], 0, 0, 0);
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the next block has landed; everyone is through with this one
    __syncthreads();
  }
  // ---- epilogue: lane (i, g) holds dQ^T [dim 16 dt + 4 g + j][query i]
  const float qsc = 0.6931471805599453f * scl[bh * 2 + 1];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int qi = q0 + qt * 16 + li;
    if (qi >= n) continue;
    float* o = dqh + ((long long)b * n + qi) * heads * hd + (long long)h * hd;
#pragma unroll
    for (int dt = 0; dt < 5; ++dt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = dt * 16 + 4 * g + j;
        if (d < hd) o[d] = acc_dq[qt][dt][j] * qsc;
      }
  }
}

// Adjoint of attn_prep on the gradients of q^ and k^.  grid (ceil(n / 64), heads, b), block 256 = 4 waves x 16 tokens, lane d holds
// channels d and d + 64, as in attn_prep.  part: [workgroup][q_norm.weight | q_norm.bias | k_norm.weight | k_norm.bias][kAttDV], the
// workgroup's 64 tokens added in token order (per wave, then wave 0..3).
__global__ __launch_bounds__(256) void attn_prep_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                            const float* __restrict__ qn_w, const float* __restrict__ kn_w, float eps,
                                                            const float* __restrict__ rope, int n_prefix, int n, int heads, int hd,
                                                            const float* __restrict__ dqh, const float* __restrict__ dkh,
                                                            float* __restrict__ dq, float* __restrict__ dk, float* __restrict__ part) {
  __shared__ float wpart[4][4][2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.y, b = blockIdx.z;
  const bool a0 = lane < hd, a1 = lane + 64 < hd;
  const float qpost = 1.4426950408889634f / sqrtf((float)hd);
  const float* xs[2] = {q, k};
  const float* gs[2] = {dqh, dkh};
  float* os[2] = {dq, dk};
  const float* ws[2] = {qn_w, kn_w};
  float lnw[2][2] = {{1.f, 1.f}, {1.f, 1.f}};
  float gw[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, gb[2][2] = {{0.f, 0.f}, {0.f, 0.f}};     // [q | k][lane | lane + 64]
#pragma unroll
  for (int s = 0; s < 2; ++s)
    if (ws[s]) {
      if (a0) lnw[s][0] = ws[s][lane];
      if (a1) lnw[s][1] = ws[s][lane + 64];
    }
  const float sgn = (lane & 1) ? 1.f : -1.f;
  for (int i = 0; i < 16; ++i) {
    const int tok = blockIdx.x * kAttBN + wave * 16 + i;
    if (tok >= n) break;
    const long long src = ((long long)b * n + tok) * heads * hd + (long long)h * hd;
    float sn0 = 0.f, cs0 = 1.f, sn1 = 0.f, cs1 = 1.f;
    const bool rot = rope != nullptr && tok >= n_prefix;
    if (rot) {
      const float* tb = rope + (long long)(tok - n_prefix) * 2 * hd;
      if (a0) { sn0 = tb[lane]; cs0 = tb[hd + lane]; }
      if (a1) { sn1 = tb[lane + 64]; cs1 = tb[hd + lane + 64]; }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float g0 = a0 ? gs[s][src + lane] : 0.f, g1 = a1 ? gs[s][src + lane + 64] : 0.f;
      if (s == 0) { g0 *= qpost; g1 *= qpost; }
      if (rot) {     // y -> y cos + sgn swap(y) sin, transposed: g -> g cos - sgn swap(g sin)
        const float t0 = dpp_quad<0xB1>(g0 * sn0), t1 = dpp_quad<0xB1>(g1 * sn1);
        g0 = g0 * cs0 - sgn * t0;
        g1 = g1 * cs1 - sgn * t1;
      }
      if (ws[s]) {   // LayerNorm backward; mean and rstd recomputed from the saved fp32 input exactly as attn_prep computes them
        const float x0 = a0 ? xs[s][src + lane] : 0.f, x1 = a1 ? xs[s][src + lane + 64] : 0.f;
        const float mean = att_wave_sum(x0 + x1) / hd;
        const float d0 = a0 ? x0 - mean : 0.f, d1 = a1 ? x1 - mean : 0.f;
        const float rstd = rsqrtf(att_wave_sum(d0 * d0 + d1 * d1) / hd + eps);
        const float xh0 = d0 * rstd, xh1 = d1 * rstd;
        gw[s][0] += g0 * xh0; gw[s][1] += g1 * xh1;
        gb[s][0] += g0; gb[s][1] += g1;
        const float e0 = g0 * lnw[s][0], e1 = g1 * lnw[s][1];
        const float m1 = att_wave_sum(e0 + e1) / hd, m2 = att_wave_sum(e0 * xh0 + e1 * xh1) / hd;
        g0 = rstd * (e0 - m1 - xh0 * m2);
        g1 = rstd * (e1 - m1 - xh1 * m2);
      }
      if (os[s]) {
        if (a0) os[s][src + lane] = g0;
        if (a1) os[s][src + lane + 64] = g1;
      }
    }
  }
  if (part == nullptr) return;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    wpart[wave][2 * s][0][lane] = gw[s][0]; wpart[wave][2 * s][1][lane] = gw[s][1];
    wpart[wave][2 * s + 1][0][lane] = gb[s][0]; wpart[wave][2 * s + 1][1][lane] = gb[s][1];
  }
  __syncthreads();
  const long long wg = ((long long)b * heads + h) * gridDim.x + blockIdx.x;
  for (int i = threadIdx.x; i < 4 * kAttDV; i += 256) {
    const int vec = i / kAttDV, d = i - vec * kAttDV;
    part[wg * (4 * kAttDV) + i] = ((wpart[0][vec][d >> 6][d & 63] + wpart[1][vec][d >> 6][d & 63]) + wpart[2][vec][d >> 6][d & 63]) +
                                  wpart[3][vec][d >> 6][d & 63];
  }
}

// grid (hd, 4), block 64: lane l adds the workgroup sums l, l + 64, ... in order, then the 64 lane sums in att_wave_sum's order
__global__ __launch_bounds__(64) void attn_norm_reduce_kernel(const float* __restrict__ part, int nwg, float* __restrict__ o0,
                                                              float* __restrict__ o1, float* __restrict__ o2, float* __restrict__ o3) {
  float* outs[4] = {o0, o1, o2, o3};
  float* o = outs[blockIdx.y];
  if (o == nullptr) return;
  float s = 0.f;
  for (int i = threadIdx.x; i < nwg; i += 64) s += part[(long long)i * (4 * kAttDV) + blockIdx.y * kAttDV + blockIdx.x];
  s = att_wave_sum(s);
  if (threadIdx.x == 0) o[blockIdx.x] = s;
}

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

AttTrainScratch attention_train_layout(void* scratch, int b, int heads, int n, int hd) {
  const size_t npad = att_npad(n), bh = (size_t)b * heads, nblk_pad = npad / kAttBN, nblk = ((size_t)n + kAttBN - 1) / kAttBN;
  const size_t rows = bh * npad * kAttKRow, rowi = bh * nblk_pad * (kAttKFrag * 512), coli = bh * nblk_pad * (kAttVFrag * 512);
  AttTrainScratch S;
  const uintptr_t base = (uintptr_t)scratch;               // (null: only the size is wanted)
  S.Qp = (f16*)base;                                       // the forward's operands where attention_operands puts them
  S.Kp = (f16*)(base + rows * sizeof(f16));
  S.Vt = (f16*)(base + (rows + rowi) * sizeof(f16));
  size_t off = up256(attention_scratch_bytes(b, heads, n));
  auto take = [&](size_t bytes) { const uintptr_t p = base + off; off += up256(bytes); return (void*)p; };
  S.Vr = (f16*)take(rowi * sizeof(f16));
  S.Kt = (f16*)take(coli * sizeof(f16));
  S.Qt = (f16*)take(coli * sizeof(f16));
  S.dOp = (f16*)take(rows * sizeof(f16));
  S.dOt = (f16*)take(coli * sizeof(f16));
  S.lsep = (float*)take(bh * npad * sizeof(float));
  S.Dp = (float*)take(bh * npad * sizeof(float));
  S.Draw = (float*)take(bh * npad * sizeof(float));
  S.amax = (float*)take(bh * nblk_pad * sizeof(float));
  S.scl = (float*)take(bh * 2 * sizeof(float));
  S.dqh = (float*)take((size_t)b * n * heads * hd * sizeof(float));
  S.dkh = (float*)take((size_t)b * n * heads * hd * sizeof(float));
  S.part = (float*)take(bh * nblk * 4 * kAttDV * sizeof(float));
  S.bytes = off;
  return S;
}

static size_t attention_train_scratch_bytes(int b, int heads, int n, int hd) { return attention_train_layout(nullptr, b, heads, n, hd).bytes; }

static hipError_t launch_attention_backward(const float* q, const float* k, const float* v, const float* qn_w, const float* qn_b, const float* kn_w,
                                            const float* kn_b, float eps, const float* rope, int n_prefix, int b, int n, int heads, int hd,
                                            const float* out, const float* lse, const float* dout, float* dq, float* dk, float* dv, float* dqn_w,
                                            float* dqn_b, float* dkn_w, float* dkn_b, void* scratch, hipStream_t st) {
  const AttTrainScratch S = attention_train_layout(scratch, b, heads, n, hd);
  const int npad = att_npad(n), nblk = (n + kAttBN - 1) / kAttBN;
  static amx::DeviceOnce attr_once;
  if (!attr_once.done()) {
    hipError_t e = hipFuncSetAttribute((const void*)attn_bwd_dkv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kDkvLds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)attn_bwd_dq_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kDqLds);
    if (e != hipSuccess) return e;
    attr_once.set();
  }
  hipError_t e = launch_attention_prep_train(q, k, v, qn_w, qn_b, kn_w, kn_b, eps, rope, n_prefix, b, n, heads, hd, S, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(attn_delta_kernel, dim3(nblk, heads, b), dim3(256), 0, st, dout, out, n, heads, hd, S.Draw, S.amax);
  hipLaunchKernelGGL(attn_dprep_kernel, dim3(npad / kAttBN, heads, b), dim3(256), 0, st, dout, lse, (const float*)S.Draw,
                     (const float*)S.amax, n, heads, hd, S.dOp, S.dOt, S.lsep, S.Dp, S.scl);
  hipLaunchKernelGGL(attn_bwd_dkv_kernel, dim3(npad / (2 * kAttBN), heads, b), dim3(256), kDkvLds, st, (const f16*)S.Qp, (const f16*)S.Kp,
                     (const f16*)S.Vr, (const f16*)S.Qt, (const f16*)S.dOp, (const f16*)S.dOt, (const float*)S.lsep, (const float*)S.Dp,
                     (const float*)S.scl, n, heads, hd, S.dkh, dv);
  const bool norm_grads = dqn_w || dqn_b || dkn_w || dkn_b;
  if (dq || dk || norm_grads) {
    hipLaunchKernelGGL(attn_bwd_dq_kernel, dim3(npad / kAttBM, heads, b), dim3(256), kDqLds, st, (const f16*)S.Qp, (const f16*)S.Kp,
                       (const f16*)S.Vr, (const f16*)S.Kt, (const f16*)S.dOp, (const float*)S.lsep, (const float*)S.Dp, (const float*)S.scl, n,
                       heads, hd, S.dqh);
    hipLaunchKernelGGL(attn_prep_bwd_kernel, dim3(nblk, heads, b), dim3(256), 0, st, q, k, qn_w, kn_w, eps, rope, n_prefix, n, heads, hd,
                       (const float*)S.dqh, (const float*)S.dkh, dq, dk, norm_grads ? S.part : (float*)nullptr);
    if (norm_grads)
      hipLaunchKernelGGL(attn_norm_reduce_kernel, dim3(hd, 4), dim3(64), 0, st, (const float*)S.part, b * heads * nblk, dqn_w, dqn_b, dkn_w,
                         dkn_b);
  }
  return hipGetLastError();
}

}  // namespace amx

using amx::fail;

extern "C" {

size_t amx_attention_train_scratch_bytes(int b, int heads, int n, int head_dim) {
  if (b < 1 || heads < 1 || n < 1 || head_dim < 2 || head_dim > 80 || (head_dim & 1)) return 0;
  return amx::attention_train_scratch_bytes(b, heads, n, head_dim);
}

int amx_attention_backward(const float* d_q, const float* d_k, const float* d_v, const float* d_qn_w, const float* d_qn_b,
                           const float* d_kn_w, const float* d_kn_b, float norm_eps, const float* d_rope, int n_prefix, int b, int n,
                           int heads, int head_dim, const float* d_out, const float* d_lse, const float* d_dout, float* d_dq, float* d_dk,
                           float* d_dv, float* d_dqn_w, float* d_dqn_b, float* d_dkn_w, float* d_dkn_b, void* d_scratch,
                           size_t scratch_bytes, void* stream) {
  if (!d_q || !d_k || !d_v || !d_out || !d_lse || !d_dout || !d_scratch) return fail(AMX_ERR_INVALID, "attention backward: null argument");
  if (int rc = amx::attention_args_ok(d_qn_w, d_qn_b, d_kn_w, d_kn_b, n_prefix, b, n, heads, head_dim)) return rc;
  if ((!d_qn_w && (d_dqn_w || d_dqn_b)) || (!d_kn_w && (d_dkn_w || d_dkn_b)))
    return fail(AMX_ERR_INVALID, "attention backward: a norm gradient was asked for a norm that is absent");
  const size_t need = amx::attention_train_scratch_bytes(b, heads, n, head_dim);
  if (scratch_bytes < need || ((uintptr_t)d_scratch & 15))
    return fail(AMX_ERR_WORKSPACE, "attention backward scratch needs %zu bytes, 16-byte aligned", need);
  AMX_HIP(amx::launch_attention_backward(d_q, d_k, d_v, d_qn_w, d_qn_b, d_kn_w, d_kn_b, norm_eps, d_rope, n_prefix, b, n, heads, head_dim,
                                         d_out, d_lse, d_dout, d_dq, d_dk, d_dv, d_dqn_w, d_dqn_b, d_dkn_w, d_dkn_b, d_scratch,
                                         (hipStream_t)stream));
  return AMX_OK;
}

}  // extern "C"
