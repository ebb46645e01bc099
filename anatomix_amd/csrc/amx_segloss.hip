// anatomix_amd -- what follows the UNet in segmentation finetuning (anatomix/segmentation/train_segmentation.py):
//   the 1x1x1 head (segmentation_utils.py:113-115) + DiceCELoss(softmax, to_onehot_y)   train_segmentation.py:105-107, :144-146
//   the validation DiceLoss                                                            train_segmentation.py:109-111, :200
//   the softmax -> argmax post-transform                                               train_segmentation.py:84-86
// fp32, planar [B][channels][V] (NCDHW), on the caller's stream without host synchronisation or allocation.  Streaming kernels,
// no MFMA: a thread owns four voxels, forms their logits in registers from the F feature rows (head mode) or reads them
// (logits mode) and never writes them.  Sums that cross workgroups go through a partial slab in the caller's scratch and a second,
// small launch that adds the slab in a fixed order in double: no float atomics, no hand-off inside a launch, results are
// bit-identical from run to run.
#include <math.h>
#include <stdio.h>

#include "amx_device.h"
#include "amx_launch.h"
#include "amx_stream.h"

namespace amx {

using Seg = StreamTile<>;                  // a thread owns four voxels of a tile of 1024 (amx_stream.h)
constexpr int kSegMaxF = 64, kSegMaxC = 32;

enum { SEG_LABEL_F32 = 0, SEG_LABEL_I64 = 1, SEG_LABEL_U8 = 2 };

// class index of a voxel, -1 when it lies outside [0, C) (NaN included); floating labels truncate toward zero as .long() does
template <int LT>
__device__ __forceinline__ int seg_label(const void* __restrict__ lab, long long i, int C) {
  if (LT == SEG_LABEL_F32) {
    const float f = ((const float*)lab)[i];
    return (f > -1.f && f < (float)C) ? (int)f : -1;
  }
  if (LT == SEG_LABEL_I64) {
    const long long l = ((const long long*)lab)[i];
    return (l >= 0 && l < C) ? (int)l : -1;
  }
  const int u = ((const unsigned char*)lab)[i];
  return u < C ? u : -1;
}

struct SegArgs {
  const float* in;        // x [B][F][V] (head mode) or z [B][C][V]
  const float* w;         // [C][F]
  const float* b;         // [C] or null
  const void* labels;     // [B][V]
  int F, C;
  long long V;
  int ntiles;             // ceil(V / Seg::kTile)
};

// head weights transposed and padded into LDS: wT[f][CP] (rows of padded classes zero), bias[CP]
template <int CP>
__device__ __forceinline__ void seg_stage_head(const SegArgs& a, float* __restrict__ wT, float* __restrict__ bias) {
  for (int i = threadIdx.x; i < a.F * CP; i += Seg::kThreads) {
    const int f = i / CP, c = i % CP;
    wT[i] = c < a.C ? a.w[c * a.F + f] : 0.f;
  }
  for (int c = threadIdx.x; c < CP; c += Seg::kThreads) bias[c] = (c < a.C && a.b) ? a.b[c] : 0.f;
}

// logits of the thread's four voxels of sample n, tile t; padded classes get -inf (softmax 0)
template <int CP, bool HEAD, bool VEC>
__device__ __forceinline__ void seg_logits(const SegArgs& a, int n, int t, const float* __restrict__ wT, const float* __restrict__ bias,
                                           float (&z)[CP][Seg::kVpt]) {
  if (HEAD) {
#pragma unroll
    for (int c = 0; c < CP; ++c)
#pragma unroll
      for (int j = 0; j < Seg::kVpt; ++j) z[c][j] = bias[c];
    const float* row = a.in + (long long)n * a.F * a.V;
    for (int f = 0; f < a.F; ++f, row += a.V) {
      float x[Seg::kVpt];
      Seg::load4<VEC>(row, t, a.V, x);
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const float wc = wT[f * CP + c];
#pragma unroll
        for (int j = 0; j < Seg::kVpt; ++j) z[c][j] += wc * x[j];
      }
    }
#pragma unroll
    for (int c = 0; c < CP; ++c)
      if (c >= a.C)
#pragma unroll
        for (int j = 0; j < Seg::kVpt; ++j) z[c][j] = -INFINITY;
  } else {
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      if (c < a.C) {
        Seg::load4<VEC>(a.in + ((long long)n * a.C + c) * a.V, t, a.V, z[c]);
      } else {
#pragma unroll
        for (int j = 0; j < Seg::kVpt; ++j) z[c][j] = -INFINITY;
      }
    }
  }
}

// softmax over the classes of one voxel, the maximum subtracted; returns log(sum exp(z - max)) and the maximum
template <int CP>
__device__ __forceinline__ void seg_softmax(const float (&z)[CP][Seg::kVpt], int j, float (&p)[CP], float& m, float& s) {
  m = z[0][j];
#pragma unroll
  for (int c = 1; c < CP; ++c) m = fmaxf(m, z[c][j]);
  s = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    p[c] = expf(z[c][j] - m);
    s += p[c];
  }
  const float inv = 1.f / s;
#pragma unroll
  for (int c = 0; c < CP; ++c) p[c] *= inv;
}

// Wave sums of N values per lane with about N + 6 shuffles instead of 6 N: step k halves the array, a lane keeping the half its
// bit k selects and handing the other half to its partner.  After log2 N steps v[0] is a partial sum of value seg_rs_index(lane)
// over the lanes that agree with this one in the low log2 N bits; the remaining steps add those up.  Fixed order.
template <int N>
__device__ __forceinline__ float seg_reduce_scatter(float (&v)[N]) {
  const int lane = threadIdx.x & 63;
  int m = 1;
#pragma unroll
  for (int half = N / 2; half >= 1; half >>= 1, m <<= 1) {
    const bool up = lane & m;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const float keep = up ? v[i + half] : v[i], send = up ? v[i] : v[i + half];
      v[i] = keep + __shfl_xor(send, m, 64);
    }
  }
  float r = v[0];
  for (; m < 64; m <<= 1) r += __shfl_xor(r, m, 64);
  return r;
}
template <int N>
__device__ __forceinline__ int seg_rs_index(int lane) {
  int c = 0, k = 0;
#pragma unroll
  for (int half = N / 2; half >= 1; half >>= 1, ++k) c += ((lane >> k) & 1) * half;
  return c;
}

// ---- statistics pass ------------------------------------------------------------------------------------------------------
// grid (nchunk, B).  One partial row per workgroup: part[(n * nchunk + chunk) * (3 C + 1)] = {I_c, P_c, G_c} per class, then the
// cross-entropy sum; badpart[n * nchunk + chunk] = labels outside [0, C).
template <int CP, bool HEAD, int LT, bool VEC>
__global__ __launch_bounds__(Seg::kThreads) void seg_stats_kernel(SegArgs a, int do_ce, float* __restrict__ part, int* __restrict__ badpart) {
  __shared__ float wT[HEAD ? kSegMaxF * CP : 1], bias[CP];
  __shared__ float red[Seg::kWaves][3 * CP + 1];
  __shared__ int redbad[Seg::kWaves];
  if (HEAD) {
    seg_stage_head<CP>(a, wT, bias);
    __syncthreads();
  }
  const int n = blockIdx.y;
  float aI[CP], aP[CP], aG[CP], ce = 0.f;
  int bad = 0;
#pragma unroll
  for (int c = 0; c < CP; ++c) aI[c] = aP[c] = aG[c] = 0.f;
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    float z[CP][Seg::kVpt];
    seg_logits<CP, HEAD, VEC>(a, n, t, wT, bias, z);
#pragma unroll
    for (int j = 0; j < Seg::kVpt; ++j) {
      const long long o = Seg::voxel<VEC>(t, j);
      if (o >= a.V) continue;
      const int lab = seg_label<LT>(a.labels, (long long)n * a.V + o, a.C);
      float p[CP], m, s;
      seg_softmax<CP>(z, j, p, m, s);
      float zl = 0.f;
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const bool hit = c == lab;
        aP[c] += p[c];
        aI[c] += hit ? p[c] : 0.f;
        aG[c] += hit ? 1.f : 0.f;
        zl = hit ? z[c][j] : zl;
      }
      if (lab < 0) ++bad;
      else if (do_ce) ce += logf(s) - (zl - m);
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    const float i = wave_reduce_xor<SumOp>(aI[c]), p = wave_reduce_xor<SumOp>(aP[c]), g = wave_reduce_xor<SumOp>(aG[c]);
    if (lane == 0) red[wave][3 * c] = i, red[wave][3 * c + 1] = p, red[wave][3 * c + 2] = g;
  }
  ce = wave_reduce_xor<SumOp>(ce);
  bad = wave_reduce_xor<SumOp>(bad);
  if (lane == 0) red[wave][3 * CP] = ce, redbad[wave] = bad;
  __syncthreads();
  const long long blk = (long long)n * gridDim.x + blockIdx.x;
  for (int k = threadIdx.x; k <= 3 * a.C; k += Seg::kThreads) {
    const int src = k == 3 * a.C ? 3 * CP : k;
    part[blk * (3 * a.C + 1) + k] = ((red[0][src] + red[1][src]) + red[2][src]) + red[3][src];
  }
  if (threadIdx.x == 0) badpart[blk] = ((redbad[0] + redbad[1]) + redbad[2]) + redbad[3];
}

struct SegLossCoef {
  int B, C, nchunk, first_class;          // first_class: 1 when the background is excluded from the Dice term
  double smooth_nr, smooth_dr, lambda_dice, lambda_ce, inv_bv;
};

// one workgroup of 16 waves: stats[B][C][3] = the slab's rows added in a fixed order in double (a wave per value, lane l taking
// chunks l, l + 64, ...), then loss[3] = {total, dice, ce} from the stored (fp32) statistics, which are what the backward reads;
// NaN when a label was out of range
constexpr int kSegFinThreads = 1024;
__global__ __launch_bounds__(kSegFinThreads) void seg_loss_finalize_kernel(const float* __restrict__ part, const int* __restrict__ badpart,
                                                                           SegLossCoef k, float* __restrict__ stats, float* __restrict__ loss,
                                                                           long long* __restrict__ bad_out) {
  __shared__ double red[kSegFinThreads];
  const int row = 3 * k.C + 1, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double ce = 0.0, bad = 0.0;
  for (int o = wave; o < k.B * row; o += kSegFinThreads / 64) {
    const int n = o / row, q = o % row;
    double s = 0.0;
    for (int ch = lane; ch < k.nchunk; ch += 64) s += (double)part[((long long)n * k.nchunk + ch) * row + q];
    s = wave_reduce_xor<SumOp>(s);
    if (lane == 0) {
      if (q == 3 * k.C) ce += s;
      else stats[(long long)n * 3 * k.C + q] = (float)s;
    }
  }
  for (int o = threadIdx.x; o < k.B * k.nchunk; o += kSegFinThreads) bad += (double)badpart[o];
  ce = block_tree_sum<double, kSegFinThreads>(ce, red);
  bad = block_tree_sum<double, kSegFinThreads>(bad, red);      // (its barriers also order the stats stores above before the reads below)
  double dice = 0.0;
  for (int o = threadIdx.x; o < k.B * k.C; o += kSegFinThreads) {
    if (o % k.C < k.first_class) continue;
    const double I = stats[3LL * o], P = stats[3LL * o + 1], G = stats[3LL * o + 2];
    dice += 1.0 - (2.0 * I + k.smooth_nr) / (G + P + k.smooth_dr);
  }
  dice = block_tree_sum<double, kSegFinThreads>(dice, red);
  if (threadIdx.x == 0) {
    const double dm = dice / ((double)k.B * (k.C - k.first_class)), cm = ce * k.inv_bv;
    const float nanv = __int_as_float(0x7fc00000);
    const bool ok = bad == 0.0;
    loss[0] = ok ? (float)(k.lambda_dice * dm + k.lambda_ce * cm) : nanv;
    loss[1] = ok ? (float)dm : nanv;
    loss[2] = ok ? (float)cm : nanv;
    *bad_out = (long long)bad;
  }
}

// ---- backward pass --------------------------------------------------------------------------------------------------------
// d loss / d z_k = gout * (lambda_dice * p_k (g_k - sum_c p_c g_c) + lambda_ce * (p_k - t_k) / (B V)),  g_c = alpha_c t_c + beta_c,
//   alpha = -2 / (N den), beta = (2 I + smooth_nr) / (N den^2), den = G + P + smooth_dr, N = B |S|; both 0 outside the class set S.
// Logits mode writes dz.  Head mode writes dx = W^T dz and one partial row {dW [C][F], db [C]} per workgroup into
// part[(n * nchunk + chunk) * (C F + C)]: per feature row the wave sums of dz_c . x_f over the wave's 256 voxels come from one
// reduce-scatter, are added into the wave's own LDS copy by CP lanes, and the four copies are added in wave order at the end.
struct SegBwdCoef {
  int first_class;
  float smooth_nr, smooth_dr, lambda_dice, ce_scale;      // ce_scale = lambda_ce / (B V)
  double inv_n;                                            // 1 / (B |S|)
};

template <int CP, bool HEAD, int LT, bool VEC>
__global__ __launch_bounds__(Seg::kThreads) void seg_backward_kernel(SegArgs a, SegBwdCoef k, const float* __restrict__ stats,
                                                                   const float* __restrict__ gout, float* __restrict__ dout,
                                                                   float* __restrict__ part) {
  __shared__ float wT[HEAD ? kSegMaxF * CP : 1], bias[CP], alpha[CP], beta[CP];
  __shared__ float accW[HEAD ? Seg::kWaves * kSegMaxF * CP : 1], accB[HEAD ? Seg::kWaves * CP : 1];
  const int n = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float g0 = *gout;
  if (HEAD) {
    seg_stage_head<CP>(a, wT, bias);
    for (int i = threadIdx.x; i < Seg::kWaves * a.F * CP; i += Seg::kThreads) accW[i] = 0.f;
    for (int i = threadIdx.x; i < Seg::kWaves * CP; i += Seg::kThreads) accB[i] = 0.f;
  }
  if ((int)threadIdx.x < CP) {
    const int c = threadIdx.x;
    float al = 0.f, be = 0.f;
    if (c >= k.first_class && c < a.C) {
      const float* s = stats + ((long long)n * a.C + c) * 3;
      const double den = (double)s[2] + (double)s[1] + (double)k.smooth_dr;
      const double sc = (double)g0 * (double)k.lambda_dice * k.inv_n;
      al = (float)(-2.0 * sc / den);
      be = (float)((2.0 * (double)s[0] + (double)k.smooth_nr) * sc / (den * den));
    }
    alpha[c] = al, beta[c] = be;
  }
  __syncthreads();
  const float cs = g0 * k.ce_scale;
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    float z[CP][Seg::kVpt];                 // logits, then d loss / d logits in place
    seg_logits<CP, HEAD, VEC>(a, n, t, wT, bias, z);
#pragma unroll
    for (int j = 0; j < Seg::kVpt; ++j) {
      const long long o = Seg::voxel<VEC>(t, j);
      if (o >= a.V) {
#pragma unroll
        for (int c = 0; c < CP; ++c) z[c][j] = 0.f;
        continue;
      }
      const int lab = seg_label<LT>(a.labels, (long long)n * a.V + o, a.C);
      float p[CP], m, s;
      seg_softmax<CP>(z, j, p, m, s);
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < CP; ++c) dot += p[c] * ((c == lab ? alpha[c] : 0.f) + beta[c]);
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const float t1 = c == lab ? 1.f : 0.f;
        z[c][j] = p[c] * ((t1 * alpha[c] + beta[c]) - dot) + cs * (p[c] - t1);
      }
    }
    if (!HEAD) {
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < a.C) Seg::store4<VEC>(dout + ((long long)n * a.C + c) * a.V, t, a.V, z[c]);
      continue;
    }
    {
      float v[CP];
#pragma unroll
      for (int c = 0; c < CP; ++c) v[c] = (z[c][0] + z[c][1]) + (z[c][2] + z[c][3]);
      const float r = seg_reduce_scatter<CP>(v);
      if (lane < CP) accB[wave * CP + seg_rs_index<CP>(lane)] += r;
    }
    const float* row = a.in + (long long)n * a.F * a.V;
    float* drow = dout + (long long)n * a.F * a.V;
    for (int f = 0; f < a.F; ++f, row += a.V, drow += a.V) {
      float x[Seg::kVpt], dx[Seg::kVpt] = {0.f, 0.f, 0.f, 0.f}, v[CP];
      Seg::load4<VEC>(row, t, a.V, x);
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const float wc = wT[f * CP + c];
#pragma unroll
        for (int j = 0; j < Seg::kVpt; ++j) dx[j] += wc * z[c][j];
        v[c] = (z[c][0] * x[0] + z[c][1] * x[1]) + (z[c][2] * x[2] + z[c][3] * x[3]);
      }
      Seg::store4<VEC>(drow, t, a.V, dx);
      const float r = seg_reduce_scatter<CP>(v);
      if (lane < CP) accW[(wave * a.F + f) * CP + seg_rs_index<CP>(lane)] += r;
    }
  }
  if (!HEAD) return;
  __syncthreads();
  const int row = a.C * a.F + a.C;
  float* dst = part + ((long long)n * gridDim.x + blockIdx.x) * row;
  for (int i = threadIdx.x; i < row; i += Seg::kThreads) {
    float s;
    if (i < a.C * a.F) {
      const int c = i / a.F, f = i % a.F;
      const float* q = accW + f * CP + c;
      const int ws = a.F * CP;
      s = ((q[0] + q[ws]) + q[2 * ws]) + q[3 * ws];
    } else {
      const float* q = accB + (i - a.C * a.F);
      s = ((q[0] + q[CP]) + q[2 * CP]) + q[3 * CP];
    }
    dst[i] = s;
  }
}

// grid (C F + C): value o of every partial row added in row order (double) -> dW [C][F] then db [C]
__global__ __launch_bounds__(Seg::kThreads) void seg_backward_finalize_kernel(const float* __restrict__ part, int nrows, int row, int cf,
                                                                            float* __restrict__ dw, float* __restrict__ db) {
  __shared__ double red[Seg::kThreads];
  const int o = blockIdx.x;
  double s = 0.0;
  for (int r = threadIdx.x; r < nrows; r += Seg::kThreads) s += (double)part[(long long)r * row + o];
  s = block_tree_sum<double, Seg::kThreads>(s, red);
  if (threadIdx.x == 0) {
    if (o < cf) dw[o] = (float)s;
    else db[o - cf] = (float)s;
  }
}

// ---- prediction -----------------------------------------------------------------------------------------------------------
// arg-max of the logits, the first maximum winning (torch.argmax on ties picks the lowest index too); uint8 [B][V]
template <int CP, bool HEAD, bool VEC>
__global__ __launch_bounds__(Seg::kThreads) void seg_argmax_kernel(SegArgs a, unsigned char* __restrict__ out) {
  __shared__ float wT[HEAD ? kSegMaxF * CP : 1], bias[CP];
  if (HEAD) {
    seg_stage_head<CP>(a, wT, bias);
    __syncthreads();
  }
  const int n = blockIdx.y;
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    float z[CP][Seg::kVpt];
    seg_logits<CP, HEAD, VEC>(a, n, t, wT, bias, z);
    unsigned char best[Seg::kVpt];
#pragma unroll
    for (int j = 0; j < Seg::kVpt; ++j) {
      float m = z[0][j];
      int bi = 0;
#pragma unroll
      for (int c = 1; c < CP; ++c)
        if (z[c][j] > m) m = z[c][j], bi = c;
      best[j] = (unsigned char)bi;
    }
    unsigned char* dst = out + (long long)n * a.V;
    Seg::store4<VEC>(dst, t, a.V, best);
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
static inline int seg_cp(int C) { return C <= 4 ? 4 : (C <= 8 ? 8 : (C <= 16 ? 16 : 32)); }
static inline bool seg_vec(long long V, const void* p0, const void* p1) { return V % 4 == 0 && aligned16(p0) && aligned16(p1); }

struct SegLayout {
  size_t part, bad, total;
};
static SegLayout seg_layout(int n, long long V, int C, int F) {
  const size_t rows = (size_t)n * Seg::chunks(n, V);
  const size_t fwd = rows * (3 * C + 1), bwd = F > 0 ? rows * ((size_t)C * F + C) : 0;
  SegLayout L;
  L.part = 0;
  L.bad = align_up((fwd > bwd ? fwd : bwd) * sizeof(float), 256);
  L.total = L.bad + align_up(rows * sizeof(int), 256);
  return L;
}
size_t seg_loss_scratch_bytes(int n, long long V, int C, int F) { return seg_layout(n, V, C, F).total; }

static SegArgs seg_args(const float* in, int F, const float* w, const float* b, const void* labels, int C, long long V) {
  SegArgs a;
  a.in = in, a.w = w, a.b = b, a.labels = labels, a.F = F, a.C = C, a.V = V, a.ntiles = (int)Seg::tiles(V);
  return a;
}

#define SEG_DISPATCH_VEC(KERNEL, CP, HEAD, LT, ...)                                                          \
  do {                                                                                                        \
    if (vec) KERNEL<CP, HEAD, LT, true><<<grid, Seg::kThreads, 0, st>>>(__VA_ARGS__);                            \
    else KERNEL<CP, HEAD, LT, false><<<grid, Seg::kThreads, 0, st>>>(__VA_ARGS__);                               \
  } while (0)
#define SEG_DISPATCH_LT(KERNEL, CP, HEAD, ...)                                                                \
  do {                                                                                                        \
    if (lt == SEG_LABEL_F32) SEG_DISPATCH_VEC(KERNEL, CP, HEAD, SEG_LABEL_F32, __VA_ARGS__);                   \
    else if (lt == SEG_LABEL_I64) SEG_DISPATCH_VEC(KERNEL, CP, HEAD, SEG_LABEL_I64, __VA_ARGS__);              \
    else SEG_DISPATCH_VEC(KERNEL, CP, HEAD, SEG_LABEL_U8, __VA_ARGS__);                                        \
  } while (0)
#define SEG_DISPATCH_HEAD(KERNEL, CP, ...)                                                                    \
  do {                                                                                                        \
    if (head) SEG_DISPATCH_LT(KERNEL, CP, true, __VA_ARGS__);                                                  \
    else SEG_DISPATCH_LT(KERNEL, CP, false, __VA_ARGS__);                                                      \
  } while (0)
#define SEG_DISPATCH(KERNEL, ...)                                                                             \
  do {                                                                                                        \
    switch (cp) {                                                                                             \
      case 4: SEG_DISPATCH_HEAD(KERNEL, 4, __VA_ARGS__); break;                                                \
      case 8: SEG_DISPATCH_HEAD(KERNEL, 8, __VA_ARGS__); break;                                                \
      case 16: SEG_DISPATCH_HEAD(KERNEL, 16, __VA_ARGS__); break;                                              \
      default: SEG_DISPATCH_HEAD(KERNEL, 32, __VA_ARGS__); break;                                              \
    }                                                                                                         \
  } while (0)

hipError_t launch_seg_loss_forward(const float* in, int F, const float* w, const float* b, const void* labels, int lt, int n, int C,
                                   long long V, int include_background, float smooth_nr, float smooth_dr, float lambda_dice,
                                   float lambda_ce, float* loss, float* stats, long long* bad, void* scratch, hipStream_t st) {
  const SegLayout L = seg_layout(n, V, C, F);
  float* part = (float*)((char*)scratch + L.part);
  int* badpart = (int*)((char*)scratch + L.bad);
  const SegArgs a = seg_args(in, F, w, b, labels, C, V);
  const int nchunk = Seg::chunks(n, V), cp = seg_cp(C), do_ce = lambda_ce != 0.f;
  const bool head = F > 0, vec = seg_vec(V, in, in);
  const dim3 grid(nchunk, n);
  SEG_DISPATCH(seg_stats_kernel, a, do_ce, part, badpart);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const SegLossCoef k = {n, C, nchunk, include_background ? 0 : 1, (double)smooth_nr, (double)smooth_dr, (double)lambda_dice,
                         (double)lambda_ce, 1.0 / ((double)n * (double)V)};
  seg_loss_finalize_kernel<<<1, kSegFinThreads, 0, st>>>(part, badpart, k, stats, loss, bad);
  return hipGetLastError();
}

hipError_t launch_seg_loss_backward(const float* in, int F, const float* w, const float* b, const void* labels, int lt, int n, int C,
                                    long long V, int include_background, float smooth_nr, float smooth_dr, float lambda_dice,
                                    float lambda_ce, const float* stats, const float* gout, float* dx, float* dw, float* db,
                                    void* scratch, hipStream_t st) {
  const SegLayout L = seg_layout(n, V, C, F);
  float* part = scratch ? (float*)((char*)scratch + L.part) : nullptr;
  const SegArgs a = seg_args(in, F, w, b, labels, C, V);
  const int nchunk = Seg::chunks(n, V), cp = seg_cp(C), first = include_background ? 0 : 1;
  const bool head = F > 0, vec = seg_vec(V, in, dx);
  const SegBwdCoef k = {first, smooth_nr, smooth_dr, lambda_dice, (float)((double)lambda_ce / ((double)n * (double)V)),
                        1.0 / ((double)n * (C - first))};
  const dim3 grid(nchunk, n);
  SEG_DISPATCH(seg_backward_kernel, a, k, stats, gout, dx, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !head) return e;
  seg_backward_finalize_kernel<<<C * F + C, Seg::kThreads, 0, st>>>(part, n * nchunk, C * F + C, C * F, dw, db);
  return hipGetLastError();
}

#undef SEG_DISPATCH_LT
#define SEG_DISPATCH_LT(KERNEL, CP, HEAD, ...)                                                                \
  do {                                                                                                        \
    if (vec) KERNEL<CP, HEAD, true><<<grid, Seg::kThreads, 0, st>>>(__VA_ARGS__);                                \
    else KERNEL<CP, HEAD, false><<<grid, Seg::kThreads, 0, st>>>(__VA_ARGS__);                                   \
  } while (0)

hipError_t launch_seg_argmax(const float* in, int F, const float* w, const float* b, int n, int C, long long V, unsigned char* out,
                             hipStream_t st) {
  const SegArgs a = seg_args(in, F, w, b, nullptr, C, V);
  const int cp = seg_cp(C);
  const bool head = F > 0, vec = V % 4 == 0 && aligned16(in) && aligned4(out);
  const dim3 grid(Seg::chunks(n, V), n);
  SEG_DISPATCH(seg_argmax_kernel, a, out);
  return hipGetLastError();
}

}  // namespace amx

namespace {
using amx::fail;

int seg_check(const void* in, int feat, const float* w, int n, int classes, long long voxels) {
  if (!in) return fail(AMX_ERR_INVALID, "null input");
  if (classes < 2 || classes > amx::kSegMaxC) return fail(AMX_ERR_INVALID, "2 <= classes <= %d (got %d)", amx::kSegMaxC, classes);
  if (feat < 0 || feat > amx::kSegMaxF)
    return fail(AMX_ERR_INVALID, "feat: 0 (logits mode) or 1 <= feat <= %d head input channels (got %d)", amx::kSegMaxF, feat);
  if (feat > 0 && !w) return fail(AMX_ERR_INVALID, "head mode needs the head weight");
  if (n < 1 || n > 65535) return fail(AMX_ERR_SHAPE, "1 <= n <= 65535 (got %d)", n);
  if (voxels < 1 || voxels >= (1LL << 40)) return fail(AMX_ERR_SHAPE, "1 <= voxels < 2^40 (got %lld)", voxels);
  return AMX_OK;
}
bool seg_finite(float v) { return v == v && v - v == 0.f; }
int seg_loss_check(const void* labels, int label_dtype, float smooth_nr, float smooth_dr, float lambda_dice, float lambda_ce) {
  if (!labels) return fail(AMX_ERR_INVALID, "null labels");
  if (label_dtype < AMX_SEG_LABEL_F32 || label_dtype > AMX_SEG_LABEL_U8)
    return fail(AMX_ERR_INVALID, "label_dtype: AMX_SEG_LABEL_F32, _I64 or _U8 (got %d)", label_dtype);
  if (!seg_finite(smooth_nr) || !seg_finite(smooth_dr) || !seg_finite(lambda_dice) || !seg_finite(lambda_ce))
    return fail(AMX_ERR_INVALID, "smooth_nr, smooth_dr, lambda_dice and lambda_ce must be finite");
  return AMX_OK;
}
}  // namespace

extern "C" {

size_t amx_seg_loss_scratch_bytes(int n, long long voxels, int classes, int feat) {
  if (n < 1 || n > 65535 || voxels < 1 || voxels >= (1LL << 40) || classes < 2 || classes > amx::kSegMaxC || feat < 0 || feat > amx::kSegMaxF)
    return 0;
  return amx::seg_loss_scratch_bytes(n, voxels, classes, feat);
}

int amx_seg_loss_forward(const float* d_in, int feat, const float* d_w, const float* d_b, const void* d_labels, int label_dtype, int n,
                         int classes, long long voxels, int include_background, float smooth_nr, float smooth_dr, float lambda_dice,
                         float lambda_ce, float* d_loss, float* d_stats, long long* d_bad_labels, void* d_scratch,
                         size_t scratch_bytes, void* stream) {
  if (int rc = seg_check(d_in, feat, d_w, n, classes, voxels)) return rc;
  if (int rc = seg_loss_check(d_labels, label_dtype, smooth_nr, smooth_dr, lambda_dice, lambda_ce)) return rc;
  if (!d_loss || !d_stats || !d_bad_labels || !d_scratch) return fail(AMX_ERR_INVALID, "null output or scratch");
  if (int rc = amx::need_scratch(amx::seg_loss_scratch_bytes(n, voxels, classes, feat), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_seg_loss_forward(d_in, feat, d_w, d_b, d_labels, label_dtype, n, classes, voxels, include_background, smooth_nr,
                                       smooth_dr, lambda_dice, lambda_ce, d_loss, d_stats, d_bad_labels, d_scratch,
                                       (hipStream_t)stream));
  return AMX_OK;
}

int amx_seg_loss_backward(const float* d_in, int feat, const float* d_w, const float* d_b, const void* d_labels, int label_dtype, int n,
                          int classes, long long voxels, int include_background, float smooth_nr, float smooth_dr, float lambda_dice,
                          float lambda_ce, const float* d_stats, const float* d_gout, float* d_dx, float* d_dw, float* d_db,
                          void* d_scratch, size_t scratch_bytes, void* stream) {
  if (int rc = seg_check(d_in, feat, d_w, n, classes, voxels)) return rc;
  if (int rc = seg_loss_check(d_labels, label_dtype, smooth_nr, smooth_dr, lambda_dice, lambda_ce)) return rc;
  if (!d_stats || !d_gout || !d_dx || d_dx == d_in) return fail(AMX_ERR_INVALID, "null argument, or d_dx aliases the input");
  if (feat > 0) {
    if (!d_dw || !d_db || !d_scratch) return fail(AMX_ERR_INVALID, "head mode needs d_dw, d_db and scratch");
    if (int rc = amx::need_scratch(amx::seg_loss_scratch_bytes(n, voxels, classes, feat), scratch_bytes)) return rc;
  }
  AMX_HIP(amx::launch_seg_loss_backward(d_in, feat, d_w, d_b, d_labels, label_dtype, n, classes, voxels, include_background, smooth_nr,
                                        smooth_dr, lambda_dice, lambda_ce, d_stats, d_gout, d_dx, d_dw, d_db, d_scratch,
                                        (hipStream_t)stream));
  return AMX_OK;
}

int amx_seg_argmax(const float* d_in, int feat, const float* d_w, const float* d_b, int n, int classes, long long voxels,
                   unsigned char* d_out, void* stream) {
  if (int rc = seg_check(d_in, feat, d_w, n, classes, voxels)) return rc;
  if (!d_out) return fail(AMX_ERR_INVALID, "null output");
  AMX_HIP(amx::launch_seg_argmax(d_in, feat, d_w, d_b, n, classes, voxels, d_out, (hipStream_t)stream));
  return AMX_OK;
}

}  // extern "C"
