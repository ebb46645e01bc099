// anatomix_amd -- bandwidth kernels around the sliding-window caller
// (monai.inferers.sliding_window_inference as used by
//  /root/reference/anatomix/registration/convex_adam_utils.py:202-219).
#include <math.h>

#include "amx_launch.h"
#include "amx_stream.h"

namespace amx {

// acc[c][v] /= cnt[v]  (the final `output_image / count_map` of sliding_window_inference)
__global__ void sw_normalize_kernel(float* __restrict__ acc, const float* __restrict__ cnt, int channels,
                                    long long voxels) {
  const long long v4n = voxels >> 2;  // float4 path; tail handled scalar
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < v4n;
       i += (long long)gridDim.x * blockDim.x) {
    const float4 c = ((const float4*)cnt)[i];
    const float4 r = make_float4(1.f / c.x, 1.f / c.y, 1.f / c.z, 1.f / c.w);
    for (int ch = 0; ch < channels; ++ch) {
      float4* p = (float4*)(acc + (long long)ch * voxels) + i;
      float4 a = *p;
      a.x *= r.x; a.y *= r.y; a.z *= r.z; a.w *= r.w;
      *p = a;
    }
  }
  if (blockIdx.x == 0)
    for (long long i = (v4n << 2) + threadIdx.x; i < voxels; i += blockDim.x)
      for (int ch = 0; ch < channels; ++ch) acc[(long long)ch * voxels + i] /= cnt[i];
}

// cnt[oz+z][oy+y][ox+x] += wmap[z][y][x]
__global__ void sw_count_kernel(float* __restrict__ cnt, int vh, int vw, int oz, int oy, int ox, int rd, int rh,
                                int rw, const float* __restrict__ wmap) {
  const long long total = (long long)rd * rh * rw;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int x = i % rw;
    const long long r = i / rw;
    const int y = r % rh;
    const int z = r / rh;
    cnt[((long long)(oz + z) * vh + (oy + y)) * vw + ox + x] += wmap[i];
  }
}

static hipError_t launch_sw_normalize(float* acc, const float* cnt, int channels, long long voxels, hipStream_t st) {
  if ((voxels & 3) && ((uintptr_t)acc & 15)) { /* alignment of channel planes is handled by the scalar tail only when voxels%4==0 */ }
  const long long v4n = voxels >> 2;
  int blocks = (int)((v4n + 255) / 256 > 4096 ? 4096 : (v4n + 255) / 256);
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(sw_normalize_kernel, dim3(blocks), dim3(256), 0, st, acc, cnt, channels, voxels);
  return hipGetLastError();
}

static hipError_t launch_sw_count(float* cnt, int vd, int vh, int vw, int oz, int oy, int ox, int rd, int rh, int rw,
                                  const float* wmap, hipStream_t st) {
  (void)vd;
  const long long total = (long long)rd * rh * rw;
  const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  hipLaunchKernelGGL(sw_count_kernel, dim3(blocks), dim3(256), 0, st, cnt, vh, vw, oz, oy, ox, rd, rh, rw, wmap);
  return hipGetLastError();
}

// ---- the window schedule ------------------------------------------------------------------------------------------------------
// registration/sliding_window.py window_starts, axis by axis: scan interval int(roi * (1 - overlap)) floored at 1 (roi itself when
// the axis equals the roi), count = 1 + the first d with d * interval + roi >= size.  AMX_OK and the plan, or AMX_ERR_SHAPE (a volume
// smaller than the roi, a non-positive size, more than kSwMaxWindows windows)
static int sw_make_plan(int vd, int vh, int vw, int rd, int rh, int rw, double overlap, SwPlan* plan) {
  const int size[3] = {vd, vh, vw}, roi[3] = {rd, rh, rw};
  long long windows = 1;
  if (!(overlap >= 0.0 && overlap < 1.0)) return fail(AMX_ERR_INVALID, "0 <= overlap < 1 (got %g)", overlap);
  for (int k = 0; k < 3; ++k) {
    if (roi[k] < 1 || size[k] < 1) return fail(AMX_ERR_SHAPE, "non-positive size (volume %d x %d x %d, roi %d x %d x %d)", vd, vh, vw, rd, rh, rw);
    if (size[k] < roi[k])
      return fail(AMX_ERR_SHAPE, "volume %d x %d x %d is smaller than the roi %d x %d x %d: pad it first", vd, vh, vw, rd, rh, rw);
    SwAxis& a = plan->ax[k];
    a.size = size[k], a.roi = roi[k];
    a.interval = size[k] == roi[k] ? roi[k] : (int)(roi[k] * (1.0 - overlap));
    if (a.interval < 1) a.interval = 1;
    a.count = (size[k] - roi[k] + a.interval - 1) / a.interval + 1;
    windows *= a.count;
    if (windows > kSwMaxWindows) return fail(AMX_ERR_SHAPE, "more than %d windows", kSwMaxWindows);
  }
  return AMX_OK;
}

// ---- count map of every window --------------------------------------------------------------------------------------------------
// windows of axis `a` that cover coordinate c: indices [lo, hi)
__device__ __forceinline__ void sw_covering(const SwAxis& a, int c, int& lo, int& hi) {
  lo = c >= a.roi ? (c - a.roi + a.interval) / a.interval : 0;       // the first i with i * interval + roi > c
  if (lo > a.count - 1) lo = a.count - 1;                            // (the last window covers the end of the axis)
  hi = lo;
  while (hi < a.count && a.start(hi) <= c) ++hi;
}

// cnt[z][y][x] = sum of wmap[z - oz][y - oy][x - ox] over the windows that cover the voxel, in window order (z outermost), plain fp32
// additions from zero: what the sequence of sw_count_kernel launches leaves on a zeroed map, bit for bit.  Writes every voxel.
__global__ __launch_bounds__(256) void sw_count_all_kernel(float* __restrict__ cnt, SwPlan p, const float* __restrict__ wmap) {
  const int vh = p.ax[1].size, vw = p.ax[2].size, rh = p.ax[1].roi, rw = p.ax[2].roi;
  const long long total = (long long)p.ax[0].size * vh * vw;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = i % vw;
    const long long r = i / vw;
    const int y = r % vh;
    const int z = r / vh;
    int z0, z1, y0, y1, x0, x1;
    sw_covering(p.ax[0], z, z0, z1);
    sw_covering(p.ax[1], y, y0, y1);
    sw_covering(p.ax[2], x, x0, x1);
    float s = 0.f;
    for (int iz = z0; iz < z1; ++iz) {
      const int wz = z - p.ax[0].start(iz);
      if (wz >= p.ax[0].roi) continue;
      for (int iy = y0; iy < y1; ++iy) {
        const int wy = y - p.ax[1].start(iy);
        if (wy >= rh) continue;
        const float* row = wmap + ((long long)wz * rh + wy) * rw;
        // eight windows of the row at a time: their loads are issued together, the additions stay in window order (a window that
        // does not cover the voxel contributes +0, which leaves the sum as it is)
        for (int ix = x0; ix < x1; ix += 8) {
          float v[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int wx = ix + k < x1 ? x - p.ax[2].start(ix + k) : rw;
            v[k] = wx < rw ? row[wx] : 0.f;
          }
#pragma unroll
          for (int k = 0; k < 8; ++k) s += v[k];
        }
      }
    }
    cnt[i] = s;
  }
}

// ---- importance map -------------------------------------------------------------------------------------------------------------
// registration/sliding_window.py importance_map: ones, or the separable Gaussian exp(-x^2 / (2 sigma^2)), x = i - (r - 1) / 2, the
// three lines multiplied first axis first, clamped below at max(min(map), 1e-3).  The minimum is the corner voxel.
__device__ __forceinline__ float sw_gauss(int i, int r, float den) {
  const float x = (float)i - (float)(r - 1) * 0.5f;
  return expf(x * x / den);
}
__global__ __launch_bounds__(256) void sw_importance_map_kernel(float* __restrict__ wmap, int rd, int rh, int rw, int gaussian, float den_z,
                                                                float den_y, float den_x) {
  const long long total = (long long)rd * rh * rw;
  const float floor_ = gaussian ? fmaxf((sw_gauss(0, rd, den_z) * sw_gauss(0, rh, den_y)) * sw_gauss(0, rw, den_x), 1e-3f) : 1.f;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = i % rw;
    const long long r = i / rw;
    const int y = r % rh;
    const int z = r / rh;
    wmap[i] = gaussian ? fmaxf((sw_gauss(z, rd, den_z) * sw_gauss(y, rh, den_y)) * sw_gauss(x, rw, den_x), floor_) : 1.f;
  }
}

// ---- finish: accumulators -> logits or labels ------------------------------------------------------------------------------------
// out = b + W (acc / cnt) per voxel, the head [C][F] transposed and padded to CP classes in LDS; a thread owns four voxels, reads
// their F accumulator values once and keeps the CP logits in registers.  LABELS: arg-max, the first maximum winning (amx_seg_argmax's
// rule), uint8; the logits are never written.  acc and cnt are only read.
using SwTile = StreamTile<>;
struct SwFinishArgs {
  const float* acc;     // [F][V]
  const float* cnt;     // [V]
  const float* w;       // [C][F]
  const float* b;       // [C] or null
  int F, C;
  long long V;
  int ntiles;
};

template <int CP, bool LABELS, bool VEC>
__global__ __launch_bounds__(SwTile::kThreads) void sw_finish_head_kernel(SwFinishArgs a, void* __restrict__ out) {
  __shared__ float wT[kSwMaxF * CP], bias[CP];
  for (int i = threadIdx.x; i < a.F * CP; i += SwTile::kThreads) {
    const int f = i / CP, c = i % CP;
    wT[i] = c < a.C ? a.w[c * a.F + f] : 0.f;
  }
  for (int c = threadIdx.x; c < CP; c += SwTile::kThreads) bias[c] = (c < a.C && a.b) ? a.b[c] : 0.f;
  __syncthreads();
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    float r[SwTile::kVpt], z[CP][SwTile::kVpt];
    SwTile::load4<VEC>(a.cnt, t, a.V, r);
#pragma unroll
    for (int j = 0; j < SwTile::kVpt; ++j) r[j] = 1.f / r[j];         // (voxels past V: never stored)
#pragma unroll
    for (int c = 0; c < CP; ++c)
#pragma unroll
      for (int j = 0; j < SwTile::kVpt; ++j) z[c][j] = bias[c];
    const float* row = a.acc;
    for (int f = 0; f < a.F; ++f, row += a.V) {
      float x[SwTile::kVpt];
      SwTile::load4<VEC>(row, t, a.V, x);
#pragma unroll
      for (int j = 0; j < SwTile::kVpt; ++j) x[j] *= r[j];
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const float wc = wT[f * CP + c];
#pragma unroll
        for (int j = 0; j < SwTile::kVpt; ++j) z[c][j] += wc * x[j];
      }
    }
    if (LABELS) {
      unsigned char best[SwTile::kVpt];
#pragma unroll
      for (int j = 0; j < SwTile::kVpt; ++j) {
        float m = z[0][j];
        int bi = 0;
#pragma unroll
        for (int c = 1; c < CP; ++c)
          if (c < a.C && z[c][j] > m) m = z[c][j], bi = c;
        best[j] = (unsigned char)bi;
      }
      SwTile::store4<VEC>((unsigned char*)out, t, a.V, best);
    } else {
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < a.C) SwTile::store4<VEC>((float*)out + (long long)c * a.V, t, a.V, z[c]);
    }
  }
}

static hipError_t launch_sw_count_all(float* cnt, const SwPlan& plan, const float* wmap, hipStream_t st) {
  const long long total = (long long)plan.ax[0].size * plan.ax[1].size * plan.ax[2].size;
  const int blocks = (int)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
  hipLaunchKernelGGL(sw_count_all_kernel, dim3(blocks), dim3(256), 0, st, cnt, plan, wmap);
  return hipGetLastError();
}

static hipError_t launch_sw_importance_map(float* wmap, int rd, int rh, int rw, int mode, double sigma_scale, hipStream_t st) {
  const long long total = (long long)rd * rh * rw;
  const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  const double sz = rd * sigma_scale, sy = rh * sigma_scale, sx = rw * sigma_scale;
  hipLaunchKernelGGL(sw_importance_map_kernel, dim3(blocks), dim3(256), 0, st, wmap, rd, rh, rw, mode == AMX_SW_MAP_GAUSSIAN ? 1 : 0,
                     (float)(-2.0 * sz * sz), (float)(-2.0 * sy * sy), (float)(-2.0 * sx * sx));
  return hipGetLastError();
}

template <int CP>
static void sw_finish_dispatch(bool labels, bool vec, int grid, hipStream_t st, const SwFinishArgs& a, void* out) {
  if (labels) {
    if (vec) sw_finish_head_kernel<CP, true, true><<<grid, SwTile::kThreads, 0, st>>>(a, out);
    else sw_finish_head_kernel<CP, true, false><<<grid, SwTile::kThreads, 0, st>>>(a, out);
  } else {
    if (vec) sw_finish_head_kernel<CP, false, true><<<grid, SwTile::kThreads, 0, st>>>(a, out);
    else sw_finish_head_kernel<CP, false, false><<<grid, SwTile::kThreads, 0, st>>>(a, out);
  }
}

// kind: AMX_SW_FEATURES (acc /= cnt in place, launch_sw_normalize's arithmetic), AMX_SW_LOGITS, AMX_SW_LABELS
static hipError_t launch_sw_finish(int kind, float* acc, const float* cnt, int feat, long long voxels, const float* w, const float* b, int classes,
                                   void* out, hipStream_t st) {
  if (kind == AMX_SW_FEATURES) return launch_sw_normalize(acc, cnt, feat, voxels, st);
  const bool labels = kind == AMX_SW_LABELS;
  SwFinishArgs a;
  a.acc = acc, a.cnt = cnt, a.w = w, a.b = b, a.F = feat, a.C = classes, a.V = voxels, a.ntiles = (int)SwTile::tiles(voxels);
  // the 16-byte path: every plane of acc (and of the logits) starts on a 16-byte boundary and holds whole quads
  const bool vec = voxels % 4 == 0 && aligned16(acc) && aligned16(cnt) && (labels ? aligned4(out) : aligned16(out));
  const int grid = a.ntiles < kStreamMaxBlocks ? a.ntiles : kStreamMaxBlocks;
  if (classes <= 4) sw_finish_dispatch<4>(labels, vec, grid, st, a, out);
  else if (classes <= 8) sw_finish_dispatch<8>(labels, vec, grid, st, a, out);
  else if (classes <= 16) sw_finish_dispatch<16>(labels, vec, grid, st, a, out);
  else sw_finish_dispatch<32>(labels, vec, grid, st, a, out);
  return hipGetLastError();
}

// ---- checks and handle state shared by the networks' window entries ------------------------------------------------------------
// AMX_OK, or AMX_ERR_INVALID for a mode that is neither constant nor gaussian, or a gaussian without a positive sigma_scale
static int sw_map_check(int mode, double sigma_scale) {
  if (mode != AMX_SW_MAP_CONSTANT && mode != AMX_SW_MAP_GAUSSIAN) return fail(AMX_ERR_INVALID, "mode: constant (0) or gaussian (1) (got %d)", mode);
  if (mode == AMX_SW_MAP_GAUSSIAN && !(sigma_scale > 0.0)) return fail(AMX_ERR_INVALID, "sigma_scale must be positive (got %g)", sigma_scale);
  return AMX_OK;
}

int sw_window_offsets(int vd, int vh, int vw, int rd, int rh, int rw, int n, const int* offsets_zyx, long long* off) {
  for (int i = 0; i < n; ++i) {
    const int oz = offsets_zyx[3 * i], oy = offsets_zyx[3 * i + 1], ox = offsets_zyx[3 * i + 2];
    if (oz < 0 || oy < 0 || ox < 0 || oz + rd > vd || oy + rh > vh || ox + rw > vw)
      return fail(AMX_ERR_SHAPE, "window (%d,%d,%d)+(%d,%d,%d) outside volume (%d,%d,%d)", oz, oy, ox, rd, rh, rw, vd, vh, vw);
    off[i] = ((long long)oz * vh + oy) * vw + ox;
  }
  return AMX_OK;
}

int SwMapCache::fetch(int rd, int rh, int rw, int mode_, double sigma_scale, hipStream_t st) {
  if (!ready) AMX_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
  const bool same_roi = map && roi[0] == rd && roi[1] == rh && roi[2] == rw;
  if (same_roi && mode == mode_ && (mode_ == AMX_SW_MAP_CONSTANT || sigma == sigma_scale)) {
    AMX_HIP(hipStreamWaitEvent(st, ready, 0));
    return AMX_OK;
  }
  const size_t bytes = (size_t)rd * rh * rw * sizeof(float);
  mode = -1;
  if (!map || (size_t)roi[0] * roi[1] * roi[2] * sizeof(float) != bytes) {
    if (map) (void)hipFree(map);     // (waits for the device: no earlier call still reads it)
    map = nullptr;
    AMX_HIP(hipMalloc((void**)&map, bytes));
  } else {
    AMX_HIP(hipStreamWaitEvent(st, ready, 0));      // rebuilt in place: after the last build, which may be on another stream
  }
  AMX_HIP(launch_sw_importance_map(map, rd, rh, rw, mode_, sigma_scale, st));
  AMX_HIP(hipEventRecord(ready, st));
  roi[0] = rd, roi[1] = rh, roi[2] = rw, mode = mode_, sigma = sigma_scale;
  return AMX_OK;
}

void SwMapCache::release() {
  if (ready) (void)hipEventDestroy(ready);
  if (map) (void)hipFree(map);
  ready = nullptr, map = nullptr, mode = -1;
}

void SwLanes::release() {
  if (stream) (void)hipStreamDestroy(stream);
  if (join) (void)hipEventDestroy(join);
  if (fork) (void)hipEventDestroy(fork);
  stream = nullptr, join = fork = nullptr;
}

// the argument check of amx_sw_finish, which sw_run makes before its first launch
static int sw_finish_check(int kind, const float* acc, const float* cnt, int feat, long long voxels, const float* w, int classes,
                           const void* out) {
  if (kind != AMX_SW_FEATURES && kind != AMX_SW_LOGITS && kind != AMX_SW_LABELS)
    return fail(AMX_ERR_INVALID, "output kind: features (0), logits (1) or labels (2) (got %d)", kind);
  if (!acc || !cnt || feat < 1 || voxels < 1 || voxels >= (1LL << 40)) return fail(AMX_ERR_INVALID, "bad argument");
  if (kind == AMX_SW_FEATURES) return AMX_OK;
  if (classes < 2 || classes > kSwMaxC) return fail(AMX_ERR_INVALID, "2 <= classes <= %d (got %d)", kSwMaxC, classes);
  if (feat > kSwMaxF) return fail(AMX_ERR_INVALID, "1 <= feat <= %d head input channels (got %d)", kSwMaxF, feat);
  if (!w || !out) return fail(AMX_ERR_INVALID, "logits and labels need the head's weight and an output buffer");
  return AMX_OK;
}

// ---- the whole-volume call ------------------------------------------------------------------------------------------------------
int sw_run(const SwNet& net, SwMapCache& cache, SwLanes* lanes, int vd, int vh, int vw, double overlap, int mode, double sigma_scale, int n_batch,
           int out_kind, const float* d_w, const float* d_b, int classes, float* d_acc, float* d_cnt, void* d_out, hipStream_t st) {
  // ---- every refusal comes before the first launch
  const int max_batch = net.max_batch < kSwMaxBatch ? net.max_batch : kSwMaxBatch;      // (kSwMaxBatch sizes the corner list of a batch)
  if (n_batch < 1 || n_batch > max_batch) return fail(AMX_ERR_INVALID, "%s1 <= n_batch <= %d (got %d)", net.prefix, max_batch, n_batch);
  if (int rc = sw_map_check(mode, sigma_scale)) return rc;
  const int rd = net.roi[0], rh = net.roi[1], rw = net.roi[2];
  SwPlan plan;
  if (int rc = sw_make_plan(vd, vh, vw, rd, rh, rw, overlap, &plan)) return rc;
  const int nwin = plan.windows(), k = n_batch < nwin ? n_batch : nwin, ngroups = (nwin + k - 1) / k;
  if (int rc = net.check(k)) return rc;
  const long long voxels = (long long)vd * vh * vw;
  if (int rc = sw_finish_check(out_kind, d_acc, d_cnt, net.channels, voxels, d_w, classes, d_out)) return rc;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  AMX_HIP(hipStreamIsCapturing(st, &cap));
  // Refused for now.  The first call allocates the cached window weights, which a capture cannot hold; and although the UNet's call
  // was written to stay on the caller's stream under capture, and each piece replays correctly on its own (count map, window
  // batches, finish), the replayed whole gave other values at every second voxel of a row when captured through
  // sliding_window_volume, and the cause is not found.  A wrong volume is worse than a refusal.
  if (cap != hipStreamCaptureStatusNone)
    return fail(AMX_ERR_INVALID, "%s cannot be captured into a graph yet: capture amx_sw_count_all, the network's forward_windows entry and "
                "amx_sw_finish, which replay correctly, or call it outside the capture", net.entry);
  // two batches in flight, as the window loop of registration/sliding_window.py keeps them
  const bool two = lanes && net.lane_groups > 0 && ngroups >= net.lane_groups;
  if (two) {
    if (!lanes->stream) AMX_HIP(hipStreamCreateWithFlags(&lanes->stream, hipStreamNonBlocking));
    if (!lanes->fork) AMX_HIP(hipEventCreateWithFlags(&lanes->fork, hipEventDisableTiming));
    if (!lanes->join) AMX_HIP(hipEventCreateWithFlags(&lanes->join, hipEventDisableTiming));
  }
  // ---- launches
  AMX_HIP(hipMemsetAsync(d_acc, 0, (size_t)net.channels * voxels * sizeof(float), st));
  if (int rc = cache.fetch(rd, rh, rw, mode, sigma_scale, st)) return rc;
  // slot 0 is the caller's stream, slot 1 the handle's: one stream more than the caller already has.  (Two streams of the handle's
  // own beside an idle caller's stream cost the overlap where a process may open four hardware queues and already uses three.)
  if (two) {
    AMX_HIP(hipEventRecord(lanes->fork, st));
    AMX_HIP(hipStreamWaitEvent(lanes->stream, lanes->fork, 0));
  }
  // the count map does not depend on the network: it runs beside the first window batch of slot 1 (it writes every voxel of d_cnt)
  AMX_HIP(launch_sw_count_all(d_cnt, plan, cache.map, st));
  int rc = AMX_OK;
  for (int g = 0; g < ngroups && rc == AMX_OK; ++g) {
    int offs[kSwMaxBatch * 3];
    const int w0 = g * k, nw = nwin - w0 < k ? nwin - w0 : k, slot = two ? g & 1 : -1;
    for (int i = 0; i < nw; ++i) plan.corner(w0 + i, offs + 3 * i);
    rc = net.run(nw, offs, slot, slot == 1 ? lanes->stream : st);
  }
  if (two) {    // joined also after a failed enqueue: the caller's stream must not run ahead of what was launched
    AMX_HIP(hipEventRecord(lanes->join, lanes->stream));
    AMX_HIP(hipStreamWaitEvent(st, lanes->join, 0));
  }
  if (rc != AMX_OK) return rc;
  AMX_HIP(launch_sw_finish(out_kind, d_acc, d_cnt, net.channels, voxels, d_w, d_b, classes, d_out, st));
  return AMX_OK;
}

}  // namespace amx

using amx::fail;

extern "C" {

int amx_sw_normalize(float* d_acc, const float* d_cnt, int channels, long long voxels, void* stream) {
  if (!d_acc || !d_cnt || channels < 1 || voxels < 1) return fail(AMX_ERR_INVALID, "bad argument");
  AMX_HIP(amx::launch_sw_normalize(d_acc, d_cnt, channels, voxels, (hipStream_t)stream));
  return AMX_OK;
}

int amx_sw_count(float* d_cnt, int vd, int vh, int vw, int oz, int oy, int ox, int rd, int rh, int rw,
                 const float* d_wmap, void* stream) {
  if (!d_cnt || !d_wmap) return fail(AMX_ERR_INVALID, "null argument");
  const int corner[3] = {oz, oy, ox};
  long long off;
  if (int rc = amx::sw_window_offsets(vd, vh, vw, rd, rh, rw, 1, corner, &off)) return rc;
  AMX_HIP(amx::launch_sw_count(d_cnt, vd, vh, vw, oz, oy, ox, rd, rh, rw, d_wmap, (hipStream_t)stream));
  return AMX_OK;
}

int amx_sw_plan(int vd, int vh, int vw, int rd, int rh, int rw, double overlap, int* offsets_zyx, int capacity) {
  if (capacity < 0 || (capacity > 0 && !offsets_zyx)) return fail(AMX_ERR_INVALID, "bad offsets buffer");
  amx::SwPlan plan;
  if (int rc = amx::sw_make_plan(vd, vh, vw, rd, rh, rw, overlap, &plan)) return rc;
  const int n = plan.windows();
  for (int i = 0; i < n && i < capacity; ++i) plan.corner(i, offsets_zyx + 3 * i);
  return n;
}

int amx_sw_importance_map(float* d_wmap, int rd, int rh, int rw, int mode, double sigma_scale, void* stream) {
  if (!d_wmap) return fail(AMX_ERR_INVALID, "null argument");
  if (rd < 1 || rh < 1 || rw < 1) return fail(AMX_ERR_SHAPE, "non-positive roi");
  if (int rc = amx::sw_map_check(mode, sigma_scale)) return rc;
  AMX_HIP(amx::launch_sw_importance_map(d_wmap, rd, rh, rw, mode, sigma_scale, (hipStream_t)stream));
  return AMX_OK;
}

int amx_sw_count_all(float* d_cnt, int vd, int vh, int vw, int rd, int rh, int rw, double overlap, const float* d_wmap,
                     void* stream) {
  if (!d_cnt || !d_wmap) return fail(AMX_ERR_INVALID, "null argument");
  amx::SwPlan plan;
  if (int rc = amx::sw_make_plan(vd, vh, vw, rd, rh, rw, overlap, &plan)) return rc;
  AMX_HIP(amx::launch_sw_count_all(d_cnt, plan, d_wmap, (hipStream_t)stream));
  return AMX_OK;
}

int amx_sw_finish(int kind, float* d_acc, const float* d_cnt, int feat, long long voxels, const float* d_w, const float* d_b,
                  int classes, void* d_out, void* stream) {
  if (int rc = amx::sw_finish_check(kind, d_acc, d_cnt, feat, voxels, d_w, classes, d_out)) return rc;
  AMX_HIP(amx::launch_sw_finish(kind, d_acc, d_cnt, feat, voxels, d_w, d_b, classes, d_out, (hipStream_t)stream));
  return AMX_OK;
}

}  // extern "C"
