// anatomix_amd -- constants, operand layouts and argument checks shared by the attention core's forward (amx_attention.hip) and
// backward (amx_attention_bwd.hip).
#pragma once
#include <stddef.h>

#include "amx_common.h"
#include "amx_launch.h"

namespace amx {

constexpr int kAttKRow = 104;         // halves per Qp / Kp row (208 B)
constexpr int kAttDV = 80;            // head_dim padded to 5 output tiles of 16
constexpr int kAttBN = 64;            // keys per block
constexpr int kAttQT = 2;             // 16-query tiles per wave (measured: QT = 1 halves the work per staged K / V tile and is slower at batch 2)
constexpr int kAttBM = 4 * 16 * kAttQT;  // queries per workgroup (4 waves)
constexpr int kAttPad = 128;          // token padding of the operand buffers
constexpr int kAttNLW = 2;            // loader waves
constexpr int kAttNBUF = 3;           // ring depth (key blocks in flight); 5 measured the same: the MFMA waves, not the loaders, set the pace
constexpr int kAttKFrag = 12;         // K fragments per key block: 4 key tiles x 3 K steps (96 padded dims), 1 KiB each
constexpr int kAttVFrag = 10;         // V^T fragments per key block: 5 output tiles x 2 K steps (64 keys)

__host__ __device__ inline int att_npad(int n) { return (n + kAttPad - 1) / kAttPad * kAttPad; }

// The two fragment images of a 64-token block (both read with one ds_read_b128 per fragment at lane * 16):
//   ROW image  (kAttKFrag fragments): token (tile tib / 16, row tib % 16), dim d -> fragment (tile, d / 32), lane ((d % 32) / 8, row),
//              element d % 8.  An MFMA operand whose K index is the feature: A of S^T = K Q^T, B of S = Q K^T.
//   COL image  (kAttVFrag fragments): dim d, token tib -> fragment (d / 16, tib / 32), lane (g, d % 16), element e, where the 32 tokens
//              of a K step are taken in the order {tile 2s tokens 4g..4g+3, tile 2s+1 tokens 4g..4g+3} -- the order an accumulator
//              tile (lane (i, g) holds rows 4g..4g+3) becomes the B operand of the next product in.  An operand whose K index is the token.
__host__ __device__ inline int att_row_idx(int tib, int d) {
  return (((tib >> 4) * 3 + (d >> 5)) * 64 + ((d & 31) >> 3) * 16 + (tib & 15)) * 8 + (d & 7);
}
__host__ __device__ inline int att_col_idx(int tib, int d) {
  const int kq = tib & 31, gq = (kq & 15) >> 2, e = (kq >> 4) * 4 + (kq & 3);
  return (((d >> 4) * 2 + (tib >> 5)) * 64 + gq * 16 + (d & 15)) * 8 + e;
}

// Scratch of the training calls: the forward's operands (attention_operands) first, then what only the backward uses.
struct AttTrainScratch {
  f16 *Qp, *Kp, *Vt;          // the forward's: Q rows [b][h][n_pad][104], K ROW image, V^T COL image (+ ones row)
  f16 *Vr, *Kt, *Qt;          // V ROW image, K^T COL image, Q^T COL image
  f16 *dOp, *dOt;             // scaled dO rows [b][h][n_pad][104] and its COL image
  float *lsep, *Dp, *Draw;    // [b][h][n_pad]: log-sum-exp (padding: huge), scaled D, unscaled D
  float *amax;                // [b][h][n_pad / 64]: max |dO| per block
  float *scl;                 // [b][h][2]: {2^-e, 2^e}
  float *dqh, *dkh;           // [b][n][heads * hd]: gradients of the prepared (normalised, rotated) q-hat / k-hat
  float *part;                // [b * heads * blocks][4][kAttDV]: per-block sums of the norm gradients
  size_t bytes;
};
AttTrainScratch attention_train_layout(void* scratch, int b, int heads, int n, int hd);
// amx_attention.hip: attn_prep with every image the backward reads
hipError_t launch_attention_prep_train(const float* q, const float* k, const float* v, const float* qn_w, const float* qn_b,
                                       const float* kn_w, const float* kn_b, float eps, const float* rope, int n_prefix, int b, int n,
                                       int heads, int hd, const AttTrainScratch& S, hipStream_t st);

// the envelope shared by the attention entries: AMX_OK or the refusal, before any launch
inline int attention_args_ok(const float* d_qn_w, const float* d_qn_b, const float* d_kn_w, const float* d_kn_b, int n_prefix, int b, int n,
                             int heads, int head_dim) {
  if (b < 1 || n < 1 || heads < 1 || head_dim < 2 || head_dim > 80 || (head_dim & 1))
    return fail(AMX_ERR_INVALID, "attention: head_dim must be even and <= 80 (got %d), b, n, heads >= 1", head_dim);
  if ((!d_qn_w) != (!d_qn_b) || (!d_kn_w) != (!d_kn_b)) return fail(AMX_ERR_INVALID, "attention: norm weight and bias go together");
  if (n_prefix < 0 || n_prefix > n) return fail(AMX_ERR_INVALID, "attention: 0 <= n_prefix <= n");
  return AMX_OK;
}
// the forward's scratch (attention_scratch_bytes), as every entry that runs the forward checks it
inline int attention_scratch_ok(const void* d_scratch, size_t scratch_bytes, int b, int heads, int n) {
  if (scratch_bytes < attention_scratch_bytes(b, heads, n) || ((uintptr_t)d_scratch & 15))
    return fail(AMX_ERR_WORKSPACE, "attention scratch needs %zu bytes, 16-byte aligned", attention_scratch_bytes(b, heads, n));
  return AMX_OK;
}

}  // namespace amx
