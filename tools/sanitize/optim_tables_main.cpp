// Host-side check of the kernel-argument tables of csrc/amx_optim.hip (amx_optim_args.h: the split of a tensor list into launches of
// <= 48 descriptors, the block prefix and its overflow check, count == 0) under the address and undefined-behaviour sanitizers.
// A stand-alone program: it launches nothing and needs no GPU.  Build and run on the build machine:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all
//         tools/sanitize/optim_tables_main.cpp -o optim_tables_check && ./optim_tables_check
// (or any C++17 compiler with -fsanitize=address,undefined).  The tables are heap blocks of exactly their size, so a read past
// the last row is reported.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../anatomix_amd/csrc/amx_optim_args.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

using namespace amx;

static long long blocks_of(long long n) { return (n + kAdamChunk - 1) / kAdamChunk; }

int main() {
  // ---- AdamW: 100 tensors -> launches of 48, 48 and 4 descriptors
  const int count = 100;
  std::vector<long long> numel(count);
  for (int t = 0; t < count; ++t) numel[t] = t % 7 == 0 ? 0 : (t % 5 == 0 ? 4096LL * t : 1 + 997LL * t);
  long long* table = (long long*)malloc(sizeof(long long) * 6 * count);
  for (int t = 0; t < count; ++t) {
    for (int k = 0; k < 5; ++k) table[t * 6 + k] = 0x1000 * (t + 1) + 16 * k;
    table[t * 6 + 5] = numel[t];
  }
  int launches = 0;
  for (int t0 = 0; t0 < count; t0 += kAdamTensors) {
    AdamArgs a;
    const int c = count - t0 < kAdamTensors ? count - t0 : kAdamTensors;
    const long long blocks = fill_adam_args(a, table, t0, c);
    long long want = 0;
    for (int t = 0; t < c; ++t) {
      CHECK(a.blk0[t] == want && a.n[t] == numel[t0 + t] && (long long)a.p[t] == table[(t0 + t) * 6]);
      want += blocks_of(numel[t0 + t]);
    }
    CHECK(blocks == want && a.count == c);
    for (int t = c; t <= kAdamTensors; ++t) CHECK(a.blk0[t] == want);
    for (int t = c; t < kAdamTensors; ++t) CHECK(a.p[t] == nullptr && a.n[t] == 0);
    ++launches;
  }
  CHECK(launches == 3);
  {
    AdamArgs a;
    CHECK(fill_adam_args(a, nullptr, 0, 0) == 0 && a.count == 0 && a.blk0[0] == 0 && a.blk0[kAdamTensors] == 0);    // count == 0
    table[5] = (kOptimMaxBlocks + 1) * (long long)kAdamChunk;                                                    // one block too many
    CHECK(fill_adam_args(a, table, 0, 48) == -1);
    table[5] = kOptimMaxBlocks * (long long)kAdamChunk;                                                          // exactly the limit ...
    table[6 + 5] = 0;
    CHECK(fill_adam_args(a, table, 0, 1) == kOptimMaxBlocks);
    table[6 + 5] = 1;                                                                                            // ... and the next tensor overflows
    CHECK(fill_adam_args(a, table, 0, 2) == -1);
  }
  free(table);

  // ---- gradient norms: the same split, partial slots numbered across the launches
  const int groups = 3;
  long long* rows = (long long*)malloc(sizeof(long long) * 3 * count);
  long long total = 0;
  for (int t = 0; t < count; ++t) {
    rows[t * 3] = 0x2000 * (t + 1) + 4;
    rows[t * 3 + 1] = numel[t];
    rows[t * 3 + 2] = t % groups;
    total += blocks_of(numel[t]);
  }
  CHECK(norm_total_blocks(rows, count, groups) == total);
  const size_t bytes = norm_scratch_bytes(total);
  char* scratch = (char*)malloc(bytes);
  long long part0 = 0;
  for (int t0 = 0; t0 < count; t0 += kAdamTensors) {
    NormArgs a;
    const int c = count - t0 < kAdamTensors ? count - t0 : kAdamTensors;
    const long long blocks = fill_norm_args(a, rows, t0, c, part0, total, scratch);
    CHECK(a.part0 == part0 && a.count == c && a.blk0[kAdamTensors] == blocks);
    for (int t = 0; t < c; ++t) CHECK(a.grp[t] == (t0 + t) % groups && a.n[t] == numel[t0 + t]);
    // every slot a block of this launch writes lies inside the scratch
    CHECK((char*)(a.part + part0 + blocks) <= (char*)a.pgrp && (char*)(a.pgrp + part0 + blocks) <= scratch + bytes);
    CHECK((char*)a.part == scratch);
    part0 += blocks;
  }
  CHECK(part0 == total);
  free(scratch);
  CHECK(norm_total_blocks(nullptr, 0, groups) == 0 && norm_scratch_bytes(0) >= 12);                               // count == 0
  {
    char one[16];
    NormArgs a;
    CHECK(fill_norm_args(a, nullptr, 0, 0, 0, 0, one) == 0 && (char*)(a.pgrp + 1) <= one + sizeof(one));
  }
  rows[2] = groups;                                                                                              // a group past the end
  CHECK(norm_total_blocks(rows, count, groups) == -1);
  rows[2] = -1;
  CHECK(norm_total_blocks(rows, count, groups) == -1);
  rows[2] = 0;
  rows[1] = -5;                                                                                                  // a negative size
  CHECK(norm_total_blocks(rows, count, groups) == -1);
  rows[1] = (kOptimMaxBlocks + 1) * (long long)kAdamChunk;
  CHECK(norm_total_blocks(rows, count, groups) == -1);
  rows[1] = kOptimMaxBlocks * (long long)kAdamChunk;
  rows[4] = 0;
  CHECK(norm_total_blocks(rows, 2, groups) == kOptimMaxBlocks);
  free(rows);
  printf("optim tables: ok\n");
  return 0;
}
