// anatomix_amd -- the kernel-argument tables of amx_optim.hip and the HOST code that fills them: the (tensor, chunk) prefix of a
// launch of <= 48 descriptors, the overflow check of its block count, the split of a longer list into launches.  Plain C++ (no
// HIP): tools/sanitize/optim_tables_main.cpp compiles this file alone under the address / undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace amx {

constexpr int kAdamTensors = 48;             // descriptors per launch: 48 x 48 B + the prefix table < the 4 KiB of kernel arguments
constexpr int kAdamChunk = 4096;             // elements per block: 256 threads x 4 x float4
constexpr long long kOptimMaxBlocks = 0x3fffffff;

struct AdamArgs {
  float* p[kAdamTensors];
  const float* g[kAdamTensors];
  float* m[kAdamTensors];
  float* v[kAdamTensors];
  const float* step[kAdamTensors];
  long long n[kAdamTensors];
  int blk0[kAdamTensors + 1];
  int count;
  int maximize;
  double lr, b1, b2;                         // for the bias corrections (torch forms them in double on the host)
  float decay, w1, b2f, w2, eps;             // 1 - lr wd, 1 - b1, b2, 1 - b2: formed in double, then rounded once, as torch's scalars are
  // non-null: {lr, beta1, beta2, eps, weight_decay} are READ FROM THE DEVICE at launch time instead of the values above -- a step
  // captured in a HIP graph then follows an lr schedule (the reference changes lr every epoch: base_model.py update_learning_rate)
  // through a captured host-to-device copy of five doubles, instead of replaying the lr that was current at capture
  const double* hyper;
};

// rows [t0, t0 + c) of `table` (6 x 64-bit {p, g, m, v, step, numel} each, c <= 48) -> a; returns the blocks of the launch, or -1
// when they overflow the grid
inline long long fill_adam_args(AdamArgs& a, const long long* table, int t0, int c) {
  long long blocks = 0;
  for (int t = 0; t < c; ++t) {
    const long long* r = table + (size_t)(t0 + t) * 6;
    a.p[t] = (float*)r[0]; a.g[t] = (const float*)r[1]; a.m[t] = (float*)r[2]; a.v[t] = (float*)r[3];
    a.step[t] = (const float*)r[4]; a.n[t] = r[5];
    a.blk0[t] = (int)blocks;
    blocks += (r[5] + kAdamChunk - 1) / kAdamChunk;
    if (blocks > kOptimMaxBlocks) return -1;
  }
  for (int t = c; t < kAdamTensors; ++t) {
    a.p[t] = nullptr; a.g[t] = nullptr; a.m[t] = nullptr; a.v[t] = nullptr; a.step[t] = nullptr; a.n[t] = 0;
  }
  for (int t = c; t <= kAdamTensors; ++t) a.blk0[t] = (int)blocks;
  a.count = c;
  return blocks;
}

// ---- gradient norms ----------------------------------------------------------------------------------------------------------
struct NormArgs {
  const float* g[kAdamTensors];
  long long n[kAdamTensors];
  int grp[kAdamTensors];
  int blk0[kAdamTensors + 1];
  int count;
  int part0;                                 // index of this launch's first block in the partial arrays
  double* part;                              // [blocks of all launches] sum of squares of a block
  int* pgrp;                                 // [blocks of all launches] its group
};

// blocks of the whole call over `count` rows of 3 x 64-bit {grad, numel, group}; -1: a negative size, a group outside
// [0, groups) or more blocks than a grid holds
inline long long norm_total_blocks(const long long* table, int count, int groups) {
  long long blocks = 0;
  for (int t = 0; t < count; ++t) {
    const long long* r = table + (size_t)t * 3;
    if (r[1] < 0 || r[2] < 0 || r[2] >= groups) return -1;
    blocks += (r[1] + kAdamChunk - 1) / kAdamChunk;
    if (blocks > kOptimMaxBlocks) return -1;
  }
  return blocks;
}

// the scratch of a call: double part[blocks], then int pgrp[blocks]; never 0 (so that a caller always has a buffer to pass)
inline size_t norm_scratch_bytes(long long blocks) { return (size_t)(blocks > 0 ? blocks : 1) * 16; }

// rows [t0, t0 + c) -> a, whose blocks start at part0 in the partial arrays; returns the blocks of this launch
inline long long fill_norm_args(NormArgs& a, const long long* table, int t0, int c, long long part0, long long total_blocks,
                                void* scratch) {
  long long blocks = 0;
  for (int t = 0; t < c; ++t) {
    const long long* r = table + (size_t)(t0 + t) * 3;
    a.g[t] = (const float*)r[0]; a.n[t] = r[1]; a.grp[t] = (int)r[2];
    a.blk0[t] = (int)blocks;
    blocks += (r[1] + kAdamChunk - 1) / kAdamChunk;
  }
  for (int t = c; t < kAdamTensors; ++t) { a.g[t] = nullptr; a.n[t] = 0; a.grp[t] = 0; }
  for (int t = c; t <= kAdamTensors; ++t) a.blk0[t] = (int)blocks;
  a.count = c;
  a.part0 = (int)part0;
  a.part = (double*)scratch;
  a.pgrp = (int*)((double*)scratch + (total_blocks > 0 ? total_blocks : 1));
  return blocks;
}

}  // namespace amx
