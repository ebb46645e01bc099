// anatomix_amd -- the optimizer of the contrastive step (pretraining/models/supcl_model.py:510-516, 584-590: torch.optim.AdamW
// over netG and over netF; stepped at supcl_model.py:628-661).  ONE launch updates every parameter tensor of an optimizer:
// the tensor descriptors travel in the kernel arguments (so a captured HIP graph replays them as they are), a block finds its
// (tensor, chunk) from a prefix table with a scalar loop.  The arithmetic follows torch's AdamW term by term:
//     p *= 1 - lr wd;  m += (g - m)(1 - b1);  v = v b2 + (1 - b2) g g;
//     p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// with the step count t read from the device (one fp32 scalar per tensor, as torch's capturable state keeps it).
//
// Gradient clipping (supcl_model.py:631-655: clip_grad_norm_(max_norm_G / max_norm_F) between unscale_ and the step) lives here
// too.  launch_grad_norms gives the L2 norm of each of `groups` lists of gradients: per-block partial sums of squares into a
// caller's scratch, then a SECOND TINY LAUNCH that adds the partials of each group in a fixed order -- not a last-block pass: a
// kernel boundary (~2 us) orders the partials without any fence, counter or spin, and the result has the same bits on every
// run and replay (no floating-point atomics anywhere).  The clipping itself costs no pass: adamw_clip_kernel reads the norm from
// the device and scales each gradient as it loads it.
#include <hip/hip_runtime.h>

#include "amx_launch.h"
#include "amx_optim_args.h"
#include "amx_stream.h"

namespace amx {

struct AdamCoef {
  float decay, w1, b1, b2, w2, inv_bc2s, eps, step_size, gsign;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamCoef& c) {
  g *= c.gsign;
  p *= c.decay;
  m = c.w1 < 0.5f ? m + c.w1 * (g - m) : g - (g - m) * c.b1;       // torch's lerp(m, g, 1 - b1), both of its branches
  v = v * c.b2 + c.w2 * g * g;
  const float denom = sqrtf(v) * c.inv_bc2s + c.eps;
  p = p - c.step_size * (m / denom);
}

// The body of both kernels.  CLIP: every gradient is first multiplied by coef = min(max_norm / (norm + 1e-6), 1), the factor of
// torch.nn.utils.clip_grad_norm_ formed as torch forms it on the device -- fp32, `max_norm / t` being t.reciprocal() * max_norm
// there, a NaN coefficient kept as torch.clamp keeps it -- with the product rounded to fp32 on its own (__fmul_rn: never
// contracted into the multiply-adds of adam_one, it is torch's separate _foreach_mul_ pass over the gradients).
template <bool CLIP>
__device__ __forceinline__ void adamw_body(const AdamArgs& a, const float* __restrict__ d_norm, float max_norm) {
  int t = 0;
  while (t + 1 < a.count && (int)blockIdx.x >= a.blk0[t + 1]) ++t;           // uniform: scalar loads from the argument segment
  const long long n = a.n[t], base = (long long)((int)blockIdx.x - a.blk0[t]) * kAdamChunk;
  float* __restrict__ p = a.p[t];
  const float* __restrict__ g = a.g[t];
  float* __restrict__ m = a.m[t];
  float* __restrict__ v = a.v[t];
  const double step = (double)*a.step[t];
  double lr = a.lr, b1 = a.b1, b2 = a.b2;
  AdamCoef c;
  c.decay = a.decay;
  c.w1 = a.w1;
  c.b2 = a.b2f;
  c.w2 = a.w2;
  c.eps = a.eps;
  if (a.hyper) {                               // same expressions as launch_adamw forms on the host, in double, rounded once
    lr = a.hyper[0]; b1 = a.hyper[1]; b2 = a.hyper[2];
    c.eps = (float)a.hyper[3];
    c.decay = (float)(1.0 - lr * a.hyper[4]);
    c.w1 = (float)(1.0 - b1);
    c.b2 = (float)b2;
    c.w2 = (float)(1.0 - b2);
  }
  const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);
  c.b1 = 1.f - c.w1;
  c.inv_bc2s = (float)(1.0 / sqrt(bc2));
  c.step_size = (float)(lr / bc1);
  c.gsign = a.maximize ? -1.f : 1.f;
  float coef = 1.f;
  if (CLIP) {
    const float q = __fmul_rn(1.0f / (*d_norm + 1e-6f), max_norm);
    coef = q > 1.f ? 1.f : q;                  // (a NaN stays a NaN)
  }
  const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
  if (vec && base + kAdamChunk <= n) {
    float4 P[4], G[4], M[4], V[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long i = base + (k * 256 + threadIdx.x) * 4;
      P[k] = *(const float4*)(p + i); G[k] = *(const float4*)(g + i); M[k] = *(const float4*)(m + i); V[k] = *(const float4*)(v + i);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (CLIP) {
        G[k].x = __fmul_rn(G[k].x, coef); G[k].y = __fmul_rn(G[k].y, coef); G[k].z = __fmul_rn(G[k].z, coef); G[k].w = __fmul_rn(G[k].w, coef);
      }
      adam_one(P[k].x, G[k].x, M[k].x, V[k].x, c);
      adam_one(P[k].y, G[k].y, M[k].y, V[k].y, c);
      adam_one(P[k].z, G[k].z, M[k].z, V[k].z, c);
      adam_one(P[k].w, G[k].w, M[k].w, V[k].w, c);
      const long long i = base + (k * 256 + threadIdx.x) * 4;
      *(float4*)(p + i) = P[k]; *(float4*)(m + i) = M[k]; *(float4*)(v + i) = V[k];
    }
    return;
  }
  const long long end = base + kAdamChunk < n ? base + kAdamChunk : n;
  for (long long i = base + threadIdx.x; i < end; i += 256) {
    float P = p[i], M = m[i], V = v[i];
    adam_one(P, CLIP ? __fmul_rn(g[i], coef) : g[i], M, V, c);
    p[i] = P; m[i] = M; v[i] = V;
  }
}

__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a) { adamw_body<false>(a, nullptr, 0.f); }

__global__ __launch_bounds__(256) void adamw_clip_kernel(AdamArgs a, const float* __restrict__ d_norm, float max_norm) {
  adamw_body<true>(a, d_norm, max_norm);
}

// table: count rows of 6 x 64-bit {p, g, m, v, step, numel} on the HOST.  d_norm non-null: the clipping step
static hipError_t launch_adamw(const long long* table, int count, double lr, double b1, double b2, double eps, double wd, int maximize,
                               hipStream_t st, const double* d_hyper = nullptr, const float* d_norm = nullptr, double max_norm = 0.0) {
  for (int t0 = 0; t0 < count; t0 += kAdamTensors) {
    AdamArgs a;
    const long long blocks = fill_adam_args(a, table, t0, count - t0 < kAdamTensors ? count - t0 : kAdamTensors);
    if (blocks < 0) return hipErrorInvalidValue;
    a.maximize = maximize; a.lr = lr; a.b1 = b1; a.b2 = b2; a.hyper = d_hyper;
    a.decay = (float)(1.0 - lr * wd); a.w1 = (float)(1.0 - b1); a.b2f = (float)b2; a.w2 = (float)(1.0 - b2); a.eps = (float)eps;
    if (blocks == 0) continue;
    if (d_norm)
      hipLaunchKernelGGL(adamw_clip_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, d_norm, (float)max_norm);
    else
      hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---- gradient norms ----------------------------------------------------------------------------------------------------------
// One block per 4096-element chunk of a tensor, found from the prefix table as above.  A thread sums the squares of its 16
// values in fp32 (15 additions), the wave adds its 64 lanes with the xor butterfly (6 more: 21 sequential fp32 additions on the
// longest path), and from there on everything is double: the four waves of the block, then the blocks of a group.
__global__ __launch_bounds__(256) void grad_sq_kernel(NormArgs a) {
  int t = 0;
  while (t + 1 < a.count && (int)blockIdx.x >= a.blk0[t + 1]) ++t;
  const long long n = a.n[t], base = (long long)((int)blockIdx.x - a.blk0[t]) * kAdamChunk;
  const float* __restrict__ g = a.g[t];
  float s = 0.f;
  if ((((uintptr_t)g) & 15) == 0 && base + kAdamChunk <= n) {
    float4 G[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) G[k] = *(const float4*)(g + base + (k * 256 + threadIdx.x) * 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s += G[k].x * G[k].x; s += G[k].y * G[k].y; s += G[k].z * G[k].z; s += G[k].w * G[k].w;
    }
  } else {
    const long long end = base + kAdamChunk < n ? base + kAdamChunk : n;
    for (long long i = base + threadIdx.x; i < end; i += 256) s += g[i] * g[i];       // <= 16 values per thread
  }
  s = wave_reduce_xor<SumOp>(s);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (double)s;
  __syncthreads();
  if (threadIdx.x == 0) {
    a.part[a.part0 + (int)blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    a.pgrp[a.part0 + (int)blockIdx.x] = a.grp[t];
  }
}

// block = group: its partials in a fixed order (thread i takes partials i, i + 256, ..., then the halving tree), in double
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ part, const int* __restrict__ pgrp, int nblocks,
                                                               float* __restrict__ out) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256)
    if (pgrp[i] == (int)blockIdx.x) acc += part[i];
  acc = block_tree_sum<double, 256>(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)sqrt(acc);
}

static size_t grad_norms_scratch_bytes(const long long* table, int count, int groups) {
  const long long blocks = norm_total_blocks(table, count, groups);
  return blocks < 0 ? 0 : norm_scratch_bytes(blocks);
}

// table: count rows of 3 x 64-bit {grad, numel, group} on the HOST
static hipError_t launch_grad_norms(const long long* table, int count, int groups, float* out, void* scratch, size_t scratch_bytes,
                                    hipStream_t st) {
  const long long total = norm_total_blocks(table, count, groups);
  if (total < 0 || scratch_bytes < norm_scratch_bytes(total)) return hipErrorInvalidValue;
  if (groups == 0) return hipSuccess;
  long long part0 = 0;
  NormArgs a;
  for (int t0 = 0; t0 < count; t0 += kAdamTensors) {
    const long long blocks = fill_norm_args(a, table, t0, count - t0 < kAdamTensors ? count - t0 : kAdamTensors, part0, total, scratch);
    if (blocks == 0) continue;
    hipLaunchKernelGGL(grad_sq_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    part0 += blocks;
  }
  fill_norm_args(a, table, 0, 0, 0, total, scratch);           // (for the two array bases)
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3((unsigned)groups), dim3(256), 0, st, a.part, a.pgrp, (int)total, out);
  return hipGetLastError();
}

}  // namespace amx

namespace {
using amx::fail;

// every row of an AdamW table: AMX_OK, or the first tensor with a null pointer or a negative size
int adamw_tensors_ok(const amx_adamw_tensor* tensors, int count) {
  for (int t = 0; t < count; ++t) {
    const amx_adamw_tensor& r = tensors[t];
    if (!r.param || !r.grad || !r.exp_avg || !r.exp_avg_sq || !r.step || r.numel < 0)
      return fail(AMX_ERR_INVALID, "adamw: tensor %d has a null pointer or a negative size", t);
  }
  return AMX_OK;
}
}  // namespace

extern "C" {

int amx_adamw_step(const amx_adamw_tensor* tensors, int count, double lr, double beta1, double beta2, double eps, double weight_decay,
                   int maximize, void* stream) {
  static_assert(sizeof(amx_adamw_tensor) == 48, "six 64-bit fields");
  if (count < 0 || (count && !tensors)) return fail(AMX_ERR_INVALID, "bad argument");
  if (!(lr >= 0.0) || !(eps >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(weight_decay >= 0.0))
    return fail(AMX_ERR_INVALID, "adamw: lr %g, betas (%g, %g), eps %g, weight_decay %g out of range", lr, beta1, beta2, eps, weight_decay);
  if (int rc = adamw_tensors_ok(tensors, count)) return rc;
  AMX_HIP(amx::launch_adamw((const long long*)tensors, count, lr, beta1, beta2, eps, weight_decay, maximize, (hipStream_t)stream));
  return AMX_OK;
}

int amx_adamw_step_dev(const amx_adamw_tensor* tensors, int count, const double* d_hyper, int maximize, void* stream) {
  if (count < 0 || (count && !tensors) || !d_hyper) return fail(AMX_ERR_INVALID, "bad argument");
  if (int rc = adamw_tensors_ok(tensors, count)) return rc;
  AMX_HIP(amx::launch_adamw((const long long*)tensors, count, 0.0, 0.0, 0.0, 0.0, 0.0, maximize, (hipStream_t)stream, d_hyper));
  return AMX_OK;
}

int amx_adamw_step_clip_dev(const amx_adamw_tensor* tensors, int count, const double* d_hyper, int maximize, const float* d_total_norm,
                            double max_norm, void* stream) {
  if (count < 0 || (count && !tensors) || !d_hyper || !d_total_norm || !(max_norm >= 0.0))
    return fail(AMX_ERR_INVALID, "adamw: bad argument (max_norm %g)", max_norm);
  if (int rc = adamw_tensors_ok(tensors, count)) return rc;
  AMX_HIP(amx::launch_adamw((const long long*)tensors, count, 0.0, 0.0, 0.0, 0.0, 0.0, maximize, (hipStream_t)stream, d_hyper, d_total_norm,
                            max_norm));
  return AMX_OK;
}

size_t amx_grad_norms_scratch_bytes(const amx_grad_tensor* tensors, int count, int groups) {
  static_assert(sizeof(amx_grad_tensor) == 24, "three 64-bit fields");
  if (count < 0 || groups < 0 || (count && !tensors)) return 0;
  return amx::grad_norms_scratch_bytes((const long long*)tensors, count, groups);
}

int amx_grad_norms(const amx_grad_tensor* tensors, int count, int groups, float* d_out, void* d_scratch, size_t scratch_bytes,
                   void* stream) {
  if (count < 0 || groups < 0 || (count && !tensors) || (groups && !d_out) || !d_scratch) return fail(AMX_ERR_INVALID, "bad argument");
  for (int t = 0; t < count; ++t)
    if (!tensors[t].grad && tensors[t].numel) return fail(AMX_ERR_INVALID, "grad_norms: tensor %d has a null pointer", t);
  if (amx_grad_norms_scratch_bytes(tensors, count, groups) == 0 || scratch_bytes < amx_grad_norms_scratch_bytes(tensors, count, groups))
    return fail(AMX_ERR_INVALID, "grad_norms: a negative size, a group outside [0, %d), too many blocks, or too little scratch", groups);
  AMX_HIP(amx::launch_grad_norms((const long long*)tensors, count, groups, d_out, d_scratch, scratch_bytes, (hipStream_t)stream));
  return AMX_OK;
}

}  // extern "C"
