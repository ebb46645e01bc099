// anatomix_amd -- C ABI (include/anatomix_amd.h): the error state (amx::fail, amx_last_error), amx_version, amx_debug_fill_lds, and
// the single-layer conv entries, which drive the launchers of several conv files at once and so belong to none of them: the
// amx_conv3d_k3_reflect* family over conv3d_single, amx_conv3d_pack_batch, amx_conv3d_upcat_merged, amx_conv3d_dgrad_interior, amx_pool2
// and their size queries.  Every other entry lives in the file that defines the launcher it calls (amx_launch.h states the rule).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "amx_launch.h"

static thread_local std::string g_err;

int amx::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

using namespace amx;   // fail and the precision helpers; launchers are written amx:: at their calls

extern "C" {

int amx_version(void) { return AMX_VERSION; }

namespace {
__global__ __launch_bounds__(256) void fill_lds_kernel(unsigned pattern, unsigned* sink) {
  extern __shared__ unsigned lds_words[];
  for (int i = threadIdx.x; i < 160 * 1024 / 4; i += 256) lds_words[i] = pattern;
  __syncthreads();
  if (sink && lds_words[(threadIdx.x * 97) % (160 * 1024 / 4)] != pattern) *sink = 1;     // (keeps the stores alive)
}
}  // namespace

int amx_debug_fill_lds(unsigned pattern, void* stream) {
  static amx::DeviceOnce attr_once;
  if (!attr_once.done()) {
    AMX_HIP(hipFuncSetAttribute((const void*)fill_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_once.set();
  }
  hipLaunchKernelGGL(fill_lds_kernel, dim3(512), dim3(256), 160 * 1024, (hipStream_t)stream, pattern, (unsigned*)nullptr);
  AMX_HIP(hipGetLastError());
  return AMX_OK;
}

const char* amx_last_error(void) { return g_err.c_str(); }

size_t amx_conv3d_packed_bytes(int cin, int cout) {
  const int cin_pad = (cin + 15) / 16 * 16;
  size_t bytes = (size_t)cout * cin_pad * 28 * 2;
  if (cin == 48 && cout == 16) bytes = (bytes + 255) / 256 * 256 + amx::conv_upcat16_packed_bytes();
  return 2 * bytes + 256;     // room for the [Wh | Wl] packing of the strict precisions (+ the block-scale words of f16x2mx)
}

// what amx_conv3d_k3_reflect_probe adds to a single-layer call: the fused max-pool output, the importance map of the fp32 planar
// epilogue, the range flag, and where the launch's name goes
struct ConvProbe {
  void* pool16;
  const float* wmap;
  int* oflow;
  char* kernel;      // 64 bytes
};

static int conv3d_single(const void* d_x0, int c0, const void* d_x1, int c1, const float* d_weight, int weight_mode,
                         int cin_real, int cout_real, const float* d_scale, const float* d_shift, int cout, int n, int d,
                         int hh, int w, int act, float slope, int precision, void* d_wpk, void* d_out16, float* d_out32,
                         void* stream, void* d_scratch = nullptr, size_t scratch_bytes = 0, const ConvProbe* probe = nullptr) {
  if (!d_x0 || (!d_weight && !(weight_mode & AMX_WEIGHTS_PREPACKED)) || !d_wpk || (!d_out16 == !d_out32)) return fail(AMX_ERR_INVALID, "bad pointer arguments");
  if (c0 % 16 || c1 % 16 || c0 + c1 < 16 || cout % 16 || cout < 16)
    return fail(AMX_ERR_INVALID, "channel counts must be multiples of 16 (c0=%d c1=%d cout=%d)", c0, c1, cout);
  if (c1 && (!d_x1 || (d & 1) || (hh & 1) || (w & 1))) return fail(AMX_ERR_SHAPE, "upsampled segment needs even dims");
  if (d < 2 || hh < 2 || w < 2) return fail(AMX_ERR_SHAPE, "reflect padding needs >= 2 voxels per axis");
  hipStream_t st = (hipStream_t)stream;
  if (precision < AMX_PREC_F16 || precision > AMX_PREC_F16X2_MX) return fail(AMX_ERR_INVALID, "unsupported precision %d", precision);
  // weight_mode | AMX_WEIGHTS_PREPACKED: d_wpk already holds this layer's packing (amx_conv3d_pack_batch), nothing is packed here
  const bool prepacked = (weight_mode & AMX_WEIGHTS_PREPACKED) != 0;
  weight_mode &= ~AMX_WEIGHTS_PREPACKED;
  if (prepacked && (is_split(precision) || d_scale)) return fail(AMX_ERR_INVALID, "prepacked weights: plain 16-bit precisions, no scale");
  if (is_mx(precision) && weight_mode != 0) return fail(AMX_ERR_INVALID, "f16x2mx packs forward weights only");
  // strict precision: x0 / x1 / out16 voxels hold [hi(C) | lo(C)]; f16x2mx: [hi(C) | lo(C) | e4m3 copies (2C bytes)] -- the INPUT
  // voxels must carry valid copies (tests/_util.py to_ndhwc_mx), the output's copy section is left untouched
  const int q = amx::conv_pick_q(cout, w, precision);
  if (d_out32 && (q > 2 || w < 32)) return fail(AMX_ERR_INVALID, "fp32 planar output needs cout <= 32 and w >= 32");
  if (cin_real < 1 || cin_real > c0 + c1 || cout_real < 1 || cout_real > cout || (weight_mode != 0 && weight_mode != 1))
    return fail(AMX_ERR_INVALID, "bad weight description (mode %d, cin_real %d, cout_real %d)", weight_mode, cin_real, cout_real);
  amx::ConvParams p;
  memset(&p, 0, sizeof p);
  if (is_mx(precision)) {
    int* mxs = (int*)((char*)d_wpk + align_up((size_t)cout * (c0 + c1) * 28 * 2 * 2, 256));
    AMX_HIP(amx::launch_pack_weights_mx(d_weight, d_scale, d_wpk, mxs, cin_real, c0 + c1, cout, q, st, cout_real));
    p.mxs = mxs;
  } else if (!prepacked) {
    AMX_HIP(amx::launch_pack_weights(d_weight, d_scale, d_wpk, cin_real, c0 + c1, cout, q, precision, st, weight_mode, cout_real));
  }
  p.N = n; p.D = d; p.H = hh; p.W = w; p.Cout = cout;
  amx::set_src0(p, d_x0, c0, d, hh, w, precision);
  if (c1) {
    amx::set_src1(p, d_x1, c1, d / 2, hh / 2, w / 2, precision);
    p.up_shift = 1;
  }
  p.wpk = (const char*)d_wpk;
  p.bias = d_shift;
  p.act = act; p.slope = slope;
  if (d_out16) {
    amx::set_out(p, d_out16, cout, d, hh, w, precision);
  } else {
    p.out32 = d_out32;
    p.py = w; p.pz = (long long)hh * w; p.pc = p.pz * d; p.pn = p.pc * cout;
  }
  amx::ConvLaunchInfo info{};
  amx::ConvLaunchInfo* const want = probe ? &info : nullptr;
  if (probe) {
    p.wmap = probe->wmap;
    p.oflow = probe->oflow;
    if (probe->wmap && !d_out32) return fail(AMX_ERR_INVALID, "the importance map belongs to the fp32 planar output");
    if (probe->pool16) {
      if (!d_out16 || !amx::conv_zmarch_can_pool(p)) return fail(AMX_ERR_SHAPE, "the fused max-pool needs a z-march layer with even extents");
      amx::set_out2(p, probe->pool16, cout, d / 2, hh / 2, w / 2, precision);
    }
  }
  if (!is_split(precision) && weight_mode == 0 && cin_real == 48 && c0 == 16 && c1 == 32 && cout == 16 && amx::conv_upcat16_eligible(p)) {
    if (prepacked)
      return fail(AMX_ERR_INVALID, "prepacked weights: the 16 + up32 -> 16 merged-tap layer packs its own format (call without the flag)");
    char* up = (char*)d_wpk + ((size_t)cout * (c0 + c1) * 28 * 2 + 255) / 256 * 256;
    AMX_HIP(amx::launch_pack_upcat16(d_weight, d_scale, up, precision, st));
    p.wpk = up;
    AMX_HIP(amx::launch_conv_upcat16(p, precision, st, want));
    if (probe && probe->kernel) memcpy(probe->kernel, info.name, sizeof info.name);
    return AMX_OK;
  }
  // split-K scratch offered by the caller (amx_conv3d_k3_reflect_ws): deep layers with few voxels split K across workgroups
  if (d_scratch && !c1 && d_out16) {
    const size_t need = amx::conv_ks_part_bytes(c0, cout, n, d, hh, w, precision, q);
    if (need && (scratch_bytes < need || ((uintptr_t)d_scratch & 15)))
      return fail(AMX_ERR_WORKSPACE, "split-K scratch needs %zu bytes, 16-byte aligned (got %zu)", need, scratch_bytes);
    if (need) p.part = (float*)d_scratch;
  }
  AMX_HIP(amx::launch_conv(p, precision, q, st, want));
  if (probe && probe->kernel) memcpy(probe->kernel, info.name, sizeof info.name);
  return AMX_OK;
}

// ---- data gradient = interior launch of the forward kernel on the zero-framed gradient + shell terms (amx_train.hip)
static bool dgrad_interior_shape_ok(int c_dy, int cout, int d, int hh, int w, int precision) {
  if (precision != AMX_PREC_F16 && precision != AMX_PREC_BF16) return false;
  amx::ConvParams p;
  memset(&p, 0, sizeof p);
  p.C0 = c_dy; p.Cout = cout; p.D = d; p.H = hh; p.W = w; p.out = (char*)1;
  return amx::conv_zmarch_eligible(p) && amx::conv_pick_q(cout, w, precision) == cout / 16 && (size_t)27 * c_dy * cout * 4 <= 150 * 1024;
}

int amx_conv3d_dgrad_interior_supported(int c_dy, int cout, int d, int hh, int w, int precision) {
  return dgrad_interior_shape_ok(c_dy, cout, d, hh, w, precision) ? 1 : 0;
}

int amx_conv3d_dgrad_interior(const void* d_dy_framed, int c_dy, const float* d_weight, int weight_flags, int cin_real, int cout_real, int cout,
                              int n, int d, int hh, int w, int precision, void* d_wpk, void* d_out16, void* stream) {
  if (!d_dy_framed || !d_wpk || !d_out16 || (!d_weight && !(weight_flags & AMX_WEIGHTS_PREPACKED)))
    return fail(AMX_ERR_INVALID, "dgrad_interior: bad pointer arguments");
  if (!dgrad_interior_shape_ok(c_dy, cout, d, hh, w, precision))
    return fail(AMX_ERR_INVALID, "dgrad_interior: shape outside the z-march kernels (ask amx_conv3d_dgrad_interior_supported)");
  if (cin_real < 1 || cin_real > c_dy || cout_real < 1 || cout_real > cout) return fail(AMX_ERR_INVALID, "dgrad_interior: bad weight description");
  hipStream_t st = (hipStream_t)stream;
  const int q = cout / 16;
  if (!(weight_flags & AMX_WEIGHTS_PREPACKED))
    AMX_HIP(amx::launch_pack_weights(d_weight, nullptr, d_wpk, cin_real, c_dy, cout, q, precision, st, 1, cout_real));
  amx::ConvParams p;
  memset(&p, 0, sizeof p);
  p.N = n; p.D = d; p.H = hh; p.W = w; p.Cout = cout; p.C0 = c_dy;
  p.s0x = (long long)c_dy * 2; p.s0y = p.s0x * (w + 4); p.s0z = p.s0y * (hh + 4); p.s0n = p.s0z * (d + 4);
  p.src0 = (const char*)d_dy_framed + 2 * (p.s0z + p.s0y + p.s0x);       // the interior of [n][d+4][hh+4][w+4][c_dy]
  p.raw_halo = 1;
  p.wpk = (const char*)d_wpk;
  p.act = AMX_ACT_NONE;
  p.out = (char*)d_out16;
  p.ox = (long long)cout * 2; p.oy = p.ox * w; p.oz = p.oy * hh; p.on = p.oz * d;
  AMX_HIP(amx::launch_conv(p, precision, q, st));
  return AMX_OK;
}

int amx_conv3d_pack_batch(const amx_pack_req* reqs, int count, int precision, void* stream) {
  if (!reqs || count < 1 || count > 256 || (precision != AMX_PREC_F16 && precision != AMX_PREC_BF16))
    return fail(AMX_ERR_INVALID, "pack_batch: bad arguments");
  std::vector<const float*> w(count);
  std::vector<void*> wpk(count);
  std::vector<int> cr(count), cp(count), co(count), q(count), md(count), cor(count);
  for (int i = 0; i < count; ++i) {
    const amx_pack_req& r = reqs[i];
    if (!r.d_weight || !r.d_wpk || r.cin_pad % 16 || r.cin_pad < 16 || r.cout % 16 || r.cout < 16 || r.cin_real < 1 || r.cin_real > r.cin_pad ||
        r.cout_real < 1 || r.cout_real > r.cout || (r.weight_mode != 0 && r.weight_mode != 1))
      return fail(AMX_ERR_INVALID, "pack_batch: bad request %d", i);
    w[i] = r.d_weight; wpk[i] = r.d_wpk; cr[i] = r.cin_real; cp[i] = r.cin_pad; co[i] = r.cout; md[i] = r.weight_mode; cor[i] = r.cout_real;
    q[i] = amx::conv_pick_q(r.cout, r.w, precision);
  }
  AMX_HIP(amx::launch_pack_weights_batch(count, w.data(), wpk.data(), cr.data(), cp.data(), co.data(), q.data(), md.data(), cor.data(), precision,
                                         (hipStream_t)stream));
  return AMX_OK;
}

size_t amx_conv3d_scratch_bytes(int c0, int c1, int cout, int n, int d, int hh, int w, int precision) {
  if (c1 || c0 % 16 || cout % 16 || precision < AMX_PREC_F16 || precision > AMX_PREC_F16X2_MX) return 0;
  return amx::conv_ks_part_bytes(c0, cout, n, d, hh, w, precision, amx::conv_pick_q(cout, w, precision));
}

int amx_conv3d_k3_reflect_ws(const void* d_x0, int c0, const void* d_x1, int c1, const float* d_weight,
                             const float* d_scale, const float* d_shift, int cout, int n, int d, int hh, int w,
                             int act, float slope, int precision, void* d_wpk, void* d_out16, float* d_out32,
                             void* d_scratch, size_t scratch_bytes, void* stream) {
  return conv3d_single(d_x0, c0, d_x1, c1, d_weight, 0, c0 + c1, cout, d_scale, d_shift, cout, n, d, hh, w, act, slope,
                       precision, d_wpk, d_out16, d_out32, stream, d_scratch, scratch_bytes);
}

int amx_conv3d_k3_reflect_probe(const void* d_x0, int c0, const void* d_x1, int c1, const float* d_weight, const float* d_scale,
                                const float* d_shift, int cout, int n, int d, int hh, int w, int act, float slope, int precision,
                                void* d_wpk, void* d_out16, float* d_out32, void* d_pool16, const float* d_wmap, int* d_oflow,
                                char* kernel_name, void* stream) {
  const ConvProbe probe{d_pool16, d_wmap, d_oflow, kernel_name};
  return conv3d_single(d_x0, c0, d_x1, c1, d_weight, 0, c0 + c1, cout, d_scale, d_shift, cout, n, d, hh, w, act, slope,
                       precision, d_wpk, d_out16, d_out32, stream, nullptr, 0, &probe);
}

int amx_conv3d_k3_reflect(const void* d_x0, int c0, const void* d_x1, int c1, const float* d_weight,
                          const float* d_scale, const float* d_shift, int cout, int n, int d, int hh, int w,
                          int act, float slope, int precision, void* d_wpk, void* d_out16, float* d_out32,
                          void* stream) {
  return conv3d_single(d_x0, c0, d_x1, c1, d_weight, 0, c0 + c1, cout, d_scale, d_shift, cout, n, d, hh, w, act, slope,
                       precision, d_wpk, d_out16, d_out32, stream);
}

int amx_conv3d_k3_reflect_ex(const void* d_x0, int c0, const void* d_x1, int c1, const float* d_weight, int weight_mode,
                             int cin_real, int cout_real, const float* d_scale, const float* d_shift, int cout, int n,
                             int d, int hh, int w, int act, float slope, int precision, void* d_wpk, void* d_out16,
                             float* d_out32, void* stream) {
  return conv3d_single(d_x0, c0, d_x1, c1, d_weight, weight_mode, cin_real, cout_real, d_scale, d_shift, cout, n, d, hh, w,
                       act, slope, precision, d_wpk, d_out16, d_out32, stream);
}

size_t amx_conv3d_upcat_merged_packed_bytes(int c0, int c1, int cout) {
  return 2 * (align_up((size_t)cout * c0 * 28 * 2, 256) + amx::conv_upmerge_packed_bytes(c1, cout, 0));   // room for [Wh | Wl]
}

int amx_conv3d_upcat_merged(const void* d_x0, int c0, const void* d_x1, int c1, const float* d_weight, const float* d_scale,
                            const float* d_shift, int cout, int n, int d, int hh, int w, int act, float slope, int precision,
                            void* d_wpk, void* d_partial, void* d_out16, void* stream) {
  if (!d_x0 || !d_x1 || !d_weight || !d_wpk || !d_partial || !d_out16) return fail(AMX_ERR_INVALID, "null argument");
  if (precision < AMX_PREC_F16 || precision > AMX_PREC_BF16X2) return fail(AMX_ERR_INVALID, "unsupported precision %d", precision);
  const bool split = is_split(precision);
  if (c0 != cout || !amx::conv_upmerge_eligible(c0, c1, cout, d, hh, w, 1, split))
    return fail(AMX_ERR_INVALID, "merged concat conv needs c0 == cout >= 32 (16 in the strict precisions), c1 %% 32 == 0, w >= 16, even dims "
                "(c0=%d c1=%d cout=%d dims %d,%d,%d)", c0, c1, cout, d, hh, w);
  hipStream_t st = (hipStream_t)stream;
  const int q = amx::conv_pick_q(cout, w, precision);
  char* wmerge = (char*)d_wpk + align_up((size_t)cout * c0 * 28 * 2 * (split ? 2 : 1), 256);
  AMX_HIP(amx::launch_pack_weights(d_weight, d_scale, d_wpk, c0, c0, cout, q, precision, st, 0, 0, c0 + c1));
  AMX_HIP(amx::launch_pack_upmerge(d_weight, d_scale, wmerge, c0, c0 + c1, c1, cout, precision, st));
  amx::ConvParams p;
  memset(&p, 0, sizeof p);
  p.N = n; p.D = d; p.H = hh; p.W = w; p.Cout = cout;
  amx::set_src0(p, d_x0, c0, d, hh, w, precision);
  p.wpk = (const char*)d_wpk; p.act = AMX_ACT_NONE;
  amx::set_out(p, d_partial, cout, d, hh, w, precision);
  AMX_HIP(amx::launch_conv(p, precision, q, st));
  amx::UpmergeParams u;
  memset(&u, 0, sizeof u);
  amx::set_src(u, d_x1, c1, d / 2, hh / 2, w / 2, precision);
  u.N = n; u.LD = d / 2; u.LH = hh / 2; u.LW = w / 2; u.Cout = cout;
  u.wpk = wmerge; u.part = (const char*)d_partial; u.out = (char*)d_out16;
  u.bias = d_shift; u.act = act; u.slope = slope;
  AMX_HIP(amx::launch_conv_upmerge(u, precision, st));
  return AMX_OK;
}

int amx_pool2(const void* d_in, void* d_out, int n, int dout, int hout, int wout, int c, int avg, int precision,
              void* stream) {
  if (!d_in || !d_out || c % 8) return fail(AMX_ERR_INVALID, "bad argument");
  AMX_HIP(amx::launch_pool2(d_in, d_out, n, dout, hout, wout, c, avg, precision, (hipStream_t)stream));
  return AMX_OK;
}

}  // extern "C"
