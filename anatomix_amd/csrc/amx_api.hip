// anatomix_amd -- C ABI (include/anatomix_amd.h) over the gfx950 kernels: the error state and the stateless operator entries.
// The UNet handle and its forward are in amx_unet.hip, the ViT in amx_vit.hip, the registration solver in amx_regsolve.hip.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "amx_gemm.h"
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

size_t amx_conv3d_dgrad_shell_scratch_bytes(void) { return amx::dgrad_shell_scratch_bytes(); }

int amx_conv3d_dgrad_fold_shell(const void* d_dy_framed, int c_dy, const float* d_weight, int co_real, int ci_real, void* d_dx, int c_dx, int n,
                                int d, int hh, int w, int precision, void* d_scratch, void* stream) {
  if (!d_dy_framed || !d_weight || !d_dx || !d_scratch || ((uintptr_t)d_scratch & 15) || co_real < 1 || co_real > c_dy || ci_real < 1 || ci_real > c_dx || d < 2 || hh < 2 || w < 2)
    return fail(AMX_ERR_INVALID, "dgrad_fold_shell: bad arguments");
  const long long fx = (long long)c_dy * 2, fy = fx * (w + 4), fz = fy * (hh + 4), fn = fz * (d + 4);
  AMX_HIP(amx::launch_dgrad_fold_shell((const char*)d_dy_framed + 2 * (fz + fy + fx), fn, fz, fy, fx, c_dy, d_weight, co_real, ci_real, d_dx, c_dx,
                                       n, d, hh, w, precision, d_scratch, (hipStream_t)stream));
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

// ---------------------------------------------------------------- training-path operators
size_t amx_train_scratch_bytes(int c) { return amx::train_scratch_bytes(c); }

int amx_bn_train_forward(const void* d_x, void* d_y, const float* d_gamma, const float* d_beta, float eps, int n,
                         long long voxels, int c, int act, float slope, void* d_scratch, float* d_save_mean,
                         float* d_save_rstd, float* d_running_mean, float* d_running_var, float momentum, int precision,
                         void* stream) {
  if (!d_x || !d_y || !d_scratch || n < 1 || voxels < 1 || c % 8 || c > 2048) return fail(AMX_ERR_INVALID, "bad argument");
  AMX_HIP(amx::launch_bn_train_forward(d_x, d_y, d_gamma, d_beta, eps, (long long)n * voxels, c, act, slope, d_scratch, d_save_mean,
                                       d_save_rstd, d_running_mean, d_running_var, momentum, precision, (hipStream_t)stream));
  return AMX_OK;
}

int amx_bn_act_backward(const void* d_dy, const void* d_y, const void* d_x, const float* d_mean, const float* d_rstd,
                        const float* d_gamma, float* d_dgamma, float* d_dbeta, void* d_dx_framed, int n, int d, int hh, int w,
                        int c, int act, float slope, void* d_scratch, int precision, void* stream) {
  if (!d_dy || !d_y || !d_dx_framed || !d_scratch || c % 8 || c > 2048) return fail(AMX_ERR_INVALID, "bad argument");
  if (d_mean && (!d_x || !d_rstd || !d_dgamma || !d_dbeta)) return fail(AMX_ERR_INVALID, "norm backward needs x, rstd, dgamma, dbeta");
  AMX_HIP(amx::launch_bn_act_backward(d_dy, d_y, d_x ? d_x : d_y, d_mean, d_rstd, d_gamma, nullptr, d_dgamma, d_dbeta, d_dx_framed, n,
                                      d, hh, w, c, act, slope, d_scratch, precision, (hipStream_t)stream));
  return AMX_OK;
}

int amx_bn_act_backward_recompute(const void* d_dy, const void* d_x, const float* d_mean, const float* d_rstd, const float* d_gamma,
                                  const float* d_beta, float* d_dgamma, float* d_dbeta, void* d_dx_framed, int n, int d, int hh, int w,
                                  int c, int act, float slope, void* d_scratch, int precision, void* stream) {
  if (!d_dy || !d_x || !d_mean || !d_rstd || !d_dgamma || !d_dbeta || !d_dx_framed || !d_scratch || c % 8 || c > 2048)
    return fail(AMX_ERR_INVALID, "bad argument");
  AMX_HIP(amx::launch_bn_act_backward(d_dy, nullptr, d_x, d_mean, d_rstd, d_gamma, d_beta, d_dgamma, d_dbeta, d_dx_framed, n, d, hh, w,
                                      c, act, slope, d_scratch, precision, (hipStream_t)stream));
  return AMX_OK;
}

int amx_pad_fold(const void* d_g_framed, void* d_din, int n, int d, int hh, int w, int c, int accumulate, int precision,
                 void* stream) {
  if (!d_g_framed || !d_din || c % 8 || d < 2 || hh < 2 || w < 2) return fail(AMX_ERR_INVALID, "bad argument");
  AMX_HIP(amx::launch_pad_fold(d_g_framed, d_din, n, d, hh, w, c, accumulate, precision, (hipStream_t)stream));
  return AMX_OK;
}

int amx_adamw_step(const amx_adamw_tensor* tensors, int count, double lr, double beta1, double beta2, double eps, double weight_decay,
                   int maximize, void* stream) {
  static_assert(sizeof(amx_adamw_tensor) == 48, "six 64-bit fields");
  if (count < 0 || (count && !tensors)) return fail(AMX_ERR_INVALID, "bad argument");
  if (!(lr >= 0.0) || !(eps >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(weight_decay >= 0.0))
    return fail(AMX_ERR_INVALID, "adamw: lr %g, betas (%g, %g), eps %g, weight_decay %g out of range", lr, beta1, beta2, eps, weight_decay);
  for (int t = 0; t < count; ++t) {
    const amx_adamw_tensor& r = tensors[t];
    if (!r.param || !r.grad || !r.exp_avg || !r.exp_avg_sq || !r.step || r.numel < 0)
      return fail(AMX_ERR_INVALID, "adamw: tensor %d has a null pointer or a negative size", t);
  }
  AMX_HIP(amx::launch_adamw((const long long*)tensors, count, lr, beta1, beta2, eps, weight_decay, maximize, (hipStream_t)stream));
  return AMX_OK;
}

int amx_adamw_step_dev(const amx_adamw_tensor* tensors, int count, const double* d_hyper, int maximize, void* stream) {
  if (count < 0 || (count && !tensors) || !d_hyper) return fail(AMX_ERR_INVALID, "bad argument");
  for (int t = 0; t < count; ++t) {
    const amx_adamw_tensor& r = tensors[t];
    if (!r.param || !r.grad || !r.exp_avg || !r.exp_avg_sq || !r.step || r.numel < 0)
      return fail(AMX_ERR_INVALID, "adamw: tensor %d has a null pointer or a negative size", t);
  }
  AMX_HIP(amx::launch_adamw((const long long*)tensors, count, 0.0, 0.0, 0.0, 0.0, 0.0, maximize, (hipStream_t)stream, d_hyper));
  return AMX_OK;
}

int amx_adamw_step_clip_dev(const amx_adamw_tensor* tensors, int count, const double* d_hyper, int maximize, const float* d_total_norm,
                            double max_norm, void* stream) {
  if (count < 0 || (count && !tensors) || !d_hyper || !d_total_norm || !(max_norm >= 0.0))
    return fail(AMX_ERR_INVALID, "adamw: bad argument (max_norm %g)", max_norm);
  for (int t = 0; t < count; ++t) {
    const amx_adamw_tensor& r = tensors[t];
    if (!r.param || !r.grad || !r.exp_avg || !r.exp_avg_sq || !r.step || r.numel < 0)
      return fail(AMX_ERR_INVALID, "adamw: tensor %d has a null pointer or a negative size", t);
  }
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

int amx_pool2_max_backward(const void* d_dp, const void* d_in, void* d_din, int n, int dout, int hout, int wout, int c,
                           int accumulate, int precision, void* stream) {
  if (!d_dp || !d_in || !d_din || c % 8) return fail(AMX_ERR_INVALID, "bad argument");
  AMX_HIP(amx::launch_pool2_max_backward(d_dp, d_in, d_din, n, dout, hout, wout, c, accumulate, precision, (hipStream_t)stream));
  return AMX_OK;
}

size_t amx_conv3d_wgrad_scratch_bytes(int n, int d, int hh, int w, int cout, int cin_pad) {
  return amx::wgrad_scratch_bytes(n, d, hh, w, cout, cin_pad);
}

int amx_conv3d_wgrad(const void* d_dy, long long dy_sn, long long dy_sz, long long dy_sy, long long dy_sx, const void* d_x0,
                     int c0, const void* d_x1, int c1, int cin_real, int cout, int n, int d, int hh, int w, float* d_dw,
                     int accumulate, void* d_scratch, size_t scratch_bytes, int precision, void* stream) {
  if (!d_dy || !d_x0 || !d_dw || !d_scratch) return fail(AMX_ERR_INVALID, "null argument");
  if (c0 % 16 || c1 % 16 || c0 + c1 < 16 || cout % 16 || cout < 16 || cin_real < 1 || cin_real > c0 + c1)
    return fail(AMX_ERR_INVALID, "channel counts must be multiples of 16 (c0=%d c1=%d cout=%d)", c0, c1, cout);
  if (c1 && (!d_x1 || (d & 1) || (hh & 1) || (w & 1))) return fail(AMX_ERR_SHAPE, "upsampled segment needs even dims");
  if (d < 2 || hh < 2 || w < 2 || w > 128) return fail(AMX_ERR_SHAPE, "wgrad supports 2 <= w <= 128 (got %d)", w);
  if (scratch_bytes < amx::wgrad_scratch_bytes(n, d, hh, w, cout, c0 + c1))
    return fail(AMX_ERR_WORKSPACE, "scratch needs %zu bytes", amx::wgrad_scratch_bytes(n, d, hh, w, cout, c0 + c1));
  amx::WgradParams p;
  memset(&p, 0, sizeof p);
  p.dy = (const char*)d_dy; p.yn = dy_sn; p.yz = dy_sz; p.yy = dy_sy; p.yx = dy_sx;
  amx::set_src0(p, d_x0, c0, d, hh, w, AMX_PREC_F16);          // 16-bit channels-last in either precision this kernel takes
  if (c1) {
    amx::set_src1(p, d_x1, c1, d / 2, hh / 2, w / 2, AMX_PREC_F16);
    p.up_shift = 1;
  }
  p.N = n; p.D = d; p.H = hh; p.W = w; p.Cout = cout;
  AMX_HIP(amx::launch_wgrad(p, cin_real, d_dw, accumulate, d_scratch, precision, (hipStream_t)stream));
  return AMX_OK;
}

size_t amx_attention_scratch_bytes(int b, int heads, int n, int head_dim) {
  if (b < 1 || heads < 1 || n < 1 || head_dim < 2 || head_dim > 80) return 0;
  return amx::attention_scratch_bytes(b, heads, n);
}

int amx_attention_qknorm_rope(const float* d_q, const float* d_k, const float* d_v, const float* d_qn_w, const float* d_qn_b,
                              const float* d_kn_w, const float* d_kn_b, float norm_eps, const float* d_rope, int n_prefix, int b,
                              int n, int heads, int head_dim, float* d_out, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (!d_q || !d_k || !d_v || !d_out || !d_scratch) return fail(AMX_ERR_INVALID, "null argument");
  if (b < 1 || n < 1 || heads < 1 || head_dim < 2 || head_dim > 80 || (head_dim & 1))
    return fail(AMX_ERR_INVALID, "attention: head_dim must be even and <= 80 (got %d), b, n, heads >= 1", head_dim);
  if ((!d_qn_w) != (!d_qn_b) || (!d_kn_w) != (!d_kn_b)) return fail(AMX_ERR_INVALID, "attention: norm weight and bias go together");
  if (n_prefix < 0 || n_prefix > n) return fail(AMX_ERR_INVALID, "attention: 0 <= n_prefix <= n");
  if (scratch_bytes < amx::attention_scratch_bytes(b, heads, n) || ((uintptr_t)d_scratch & 15))
    return fail(AMX_ERR_WORKSPACE, "attention scratch needs %zu bytes, 16-byte aligned", amx::attention_scratch_bytes(b, heads, n));
  AMX_HIP(amx::launch_attention(d_q, d_k, d_v, d_qn_w, d_qn_b, d_kn_w, d_kn_b, norm_eps, d_rope, n_prefix, b, n, heads, head_dim, d_out,
                                d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

int amx_attention_prepared(const void* d_scratch, size_t scratch_bytes, int b, int n, int heads, int head_dim, float* d_out, void* stream) {
  if (!d_scratch || !d_out) return fail(AMX_ERR_INVALID, "null argument");
  if (b < 1 || n < 1 || heads < 1 || head_dim < 2 || head_dim > 80 || (head_dim & 1))
    return fail(AMX_ERR_INVALID, "attention: head_dim must be even and <= 80 (got %d), b, n, heads >= 1", head_dim);
  if (scratch_bytes < amx::attention_scratch_bytes(b, heads, n) || ((uintptr_t)d_scratch & 15))
    return fail(AMX_ERR_WORKSPACE, "attention scratch needs %zu bytes, 16-byte aligned", amx::attention_scratch_bytes(b, heads, n));
  void *Qp, *Kp, *Vt;
  amx::attention_operands((void*)d_scratch, b, heads, n, &Qp, &Kp, &Vt, nullptr, nullptr);
  AMX_HIP(amx::launch_attention_fwd(Qp, Kp, Vt, b, n, heads, head_dim, d_out, (hipStream_t)stream));
  return AMX_OK;
}

namespace {
// the envelope shared by the attention entries: AMX_OK or the refusal, before any launch
int attention_args_ok(const float* d_qn_w, const float* d_qn_b, const float* d_kn_w, const float* d_kn_b, int n_prefix, int b, int n,
                      int heads, int head_dim) {
  if (b < 1 || n < 1 || heads < 1 || head_dim < 2 || head_dim > 80 || (head_dim & 1))
    return fail(AMX_ERR_INVALID, "attention: head_dim must be even and <= 80 (got %d), b, n, heads >= 1", head_dim);
  if ((!d_qn_w) != (!d_qn_b) || (!d_kn_w) != (!d_kn_b)) return fail(AMX_ERR_INVALID, "attention: norm weight and bias go together");
  if (n_prefix < 0 || n_prefix > n) return fail(AMX_ERR_INVALID, "attention: 0 <= n_prefix <= n");
  return AMX_OK;
}
}  // namespace

size_t amx_attention_train_scratch_bytes(int b, int heads, int n, int head_dim) {
  if (b < 1 || heads < 1 || n < 1 || head_dim < 2 || head_dim > 80 || (head_dim & 1)) return 0;
  return amx::attention_train_scratch_bytes(b, heads, n, head_dim);
}

int amx_attention_qknorm_rope_train(const float* d_q, const float* d_k, const float* d_v, const float* d_qn_w, const float* d_qn_b,
                                    const float* d_kn_w, const float* d_kn_b, float norm_eps, const float* d_rope, int n_prefix, int b,
                                    int n, int heads, int head_dim, float* d_out, float* d_lse, void* d_scratch, size_t scratch_bytes,
                                    void* stream) {
  if (!d_q || !d_k || !d_v || !d_out || !d_lse || !d_scratch) return fail(AMX_ERR_INVALID, "attention: null argument");
  if (int rc = attention_args_ok(d_qn_w, d_qn_b, d_kn_w, d_kn_b, n_prefix, b, n, heads, head_dim)) return rc;
  if (scratch_bytes < amx::attention_scratch_bytes(b, heads, n) || ((uintptr_t)d_scratch & 15))
    return fail(AMX_ERR_WORKSPACE, "attention scratch needs %zu bytes, 16-byte aligned", amx::attention_scratch_bytes(b, heads, n));
  AMX_HIP(amx::launch_attention(d_q, d_k, d_v, d_qn_w, d_qn_b, d_kn_w, d_kn_b, norm_eps, d_rope, n_prefix, b, n, heads, head_dim, d_out,
                                d_scratch, (hipStream_t)stream, d_lse));
  return AMX_OK;
}

int amx_attention_backward(const float* d_q, const float* d_k, const float* d_v, const float* d_qn_w, const float* d_qn_b,
                           const float* d_kn_w, const float* d_kn_b, float norm_eps, const float* d_rope, int n_prefix, int b, int n,
                           int heads, int head_dim, const float* d_out, const float* d_lse, const float* d_dout, float* d_dq, float* d_dk,
                           float* d_dv, float* d_dqn_w, float* d_dqn_b, float* d_dkn_w, float* d_dkn_b, void* d_scratch,
                           size_t scratch_bytes, void* stream) {
  if (!d_q || !d_k || !d_v || !d_out || !d_lse || !d_dout || !d_scratch) return fail(AMX_ERR_INVALID, "attention backward: null argument");
  if (int rc = attention_args_ok(d_qn_w, d_qn_b, d_kn_w, d_kn_b, n_prefix, b, n, heads, head_dim)) return rc;
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

size_t amx_linear_train_scratch_bytes(long long m, int k, int n) { return amx::linear_train_scratch_bytes(m, k, n); }

namespace {
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

size_t amx_supcon_scratch_bytes(int n, int c) { return amx::supcon_scratch_bytes(n, c); }

int amx_supcon_loss(const float* d_feat, const int* d_labels, int n, int c, float temperature, int weigh_rarity,
                    int balance_denominator, int sqrt_mode, float* d_loss, float* d_grad, void* d_scratch,
                    size_t scratch_bytes, void* stream) {
  if (!d_feat || !d_labels || !d_loss || !d_scratch) return fail(AMX_ERR_INVALID, "null argument");
  if (n < 2 || n > 16384 || c < 1 || !(temperature > 0.f)) return fail(AMX_ERR_INVALID, "bad sizes (n=%d c=%d T=%g)", n, c, temperature);
  if (int rc = amx::need_scratch(amx::supcon_scratch_bytes(n, c), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_supcon(d_feat, d_labels, n, c, temperature, weigh_rarity, balance_denominator, sqrt_mode, d_loss,
                             d_grad, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

size_t amx_instance_norm_scratch_bytes(int n, int c) { return amx::instnorm_scratch_bytes(n, c, 0); }

int amx_instance_norm(void* d_x, const float* d_gamma, const float* d_beta, float eps, int n, long long voxels, int c,
                      int act, float slope, void* d_scratch, int precision, void* stream) {
  if (!d_x || !d_scratch || c % 8 || c > 2048 || n < 1 || voxels < 1) return fail(AMX_ERR_INVALID, "bad argument");
  if (!d_gamma != !d_beta) return fail(AMX_ERR_INVALID, "gamma and beta come together");
  // f16x2mx (row-planar layout): this entry has no row length -- a sample is taken as ONE row of `voxels` voxels
  if (precision == AMX_PREC_F16X2_MX && voxels > (1 << 24)) return fail(AMX_ERR_INVALID, "f16x2mx: at most 2^24 voxels per sample here");
  AMX_HIP(amx::launch_instnorm(d_x, d_gamma, d_beta, eps, n, voxels, c, act, slope, d_scratch, precision,
                               (hipStream_t)stream, nullptr, 0, nullptr, (int)voxels));
  return AMX_OK;
}

int amx_upsample2_trilinear(const void* d_in, void* d_out, int n, int din, int hin, int win, int c, int precision,
                            void* stream) {
  if (!d_in || !d_out || c % 8 || n < 1 || din < 1 || hin < 1 || win < 1) return fail(AMX_ERR_INVALID, "bad argument");
  AMX_HIP(amx::launch_upsample2_trilinear(d_in, d_out, n, din, hin, win, c, precision, (hipStream_t)stream));
  return AMX_OK;
}

size_t amx_mindssc_scratch_bytes(int H, int W, int D) { return amx::mindssc_scratch_bytes(H, W, D); }

int amx_mindssc(const float* d_img, int H, int W, int D, int radius, int dilation, float* d_out, void* d_scratch,
                size_t scratch_bytes, void* stream) {
  if (!d_img || !d_out || !d_scratch) return fail(AMX_ERR_INVALID, "null argument");
  if (H < 1 || W < 1 || D < 1) return fail(AMX_ERR_SHAPE, "non-positive shape");
  if (radius < 1 || radius > 2 || dilation < 1 || dilation > 4)
    return fail(AMX_ERR_INVALID, "radius in {1, 2}, dilation in [1, 4] (got %d, %d)", radius, dilation);
  if (int rc = amx::need_scratch(amx::mindssc_scratch_bytes(H, W, D), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_mindssc(d_img, H, W, D, radius, dilation, d_out, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

int amx_avg_pool3d_cat(const float* d_a, int ca, float scale_a, const float* d_b, int cb, float scale_b, int H, int W, int D,
                       int g, float* d_out, void* stream) {
  if (!d_out || (ca > 0 && !d_a) || (cb > 0 && !d_b) || ca < 0 || cb < 0 || ca + cb < 1) return fail(AMX_ERR_INVALID, "bad argument");
  if (g < 1 || H < g || W < g || D < g) return fail(AMX_ERR_SHAPE, "pool size %d does not fit (%d,%d,%d)", g, H, W, D);
  AMX_HIP(amx::launch_pool_cat(d_a, ca, scale_a, d_b, cb, scale_b, H, W, D, g, d_out, (hipStream_t)stream));
  return AMX_OK;
}

int amx_box_filter3d(const float* d_in, float* d_out, int c, int H, int W, int D, int k, void* stream) {
  if (!d_in || !d_out || d_in == d_out || c < 1 || c > 65535) return fail(AMX_ERR_INVALID, "bad argument");
  if (H < 1 || W < 1 || D < 1) return fail(AMX_ERR_SHAPE, "non-positive shape");
  if (k < 3 || k > 9 || !(k & 1)) return fail(AMX_ERR_INVALID, "kernel size must be odd in [3, 9] (got %d)", k);
  AMX_HIP(amx::launch_box_filter(d_in, d_out, c, H, W, D, k, (hipStream_t)stream));
  return AMX_OK;
}

size_t amx_correlate_scratch_bytes(int h, int w, int d, int disp_hw) { return amx::correlate_scratch_bytes(h, w, d, disp_hw); }

int amx_correlate_ssd(const float* d_fix, const float* d_mov, int c, int h, int w, int d, int disp_hw, float* d_ssd,
                      long long* d_argmin, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (!d_fix || !d_mov || !d_ssd || !d_scratch || c < 1) return fail(AMX_ERR_INVALID, "bad argument");
  if (h < 1 || w < 1 || d < 1) return fail(AMX_ERR_SHAPE, "non-positive shape");
  if (disp_hw < 1 || disp_hw > 3) return fail(AMX_ERR_INVALID, "disp_hw in {1, 2, 3} (got %d)", disp_hw);
  if (int rc = amx::need_scratch(amx::correlate_scratch_bytes(h, w, d, disp_hw), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_correlate(d_fix, d_mov, c, h, w, d, disp_hw, d_ssd, d_argmin, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

static int mlp_check(int n, int cin, int width, int n_layers) {
  if (n < 1 || n > 2048) return fail(AMX_ERR_SHAPE, "mlp head: 1 <= n <= 2048 rows (got %d)", n);
  if (cin < 4 || cin % 4 || width < 8 || width % 8) return fail(AMX_ERR_SHAPE, "mlp head: cin %% 4 == 0 and width %% 8 == 0 (got %d, %d)", cin, width);
  if (cin > 4096 || width > 4096) return fail(AMX_ERR_SHAPE, "mlp head: at most 4096 features per layer (got %d, %d)", cin, width);
  if (n_layers < 1 || n_layers > 8) return fail(AMX_ERR_INVALID, "mlp head: 1 <= n_layers <= 8 (got %d)", n_layers);
  return AMX_OK;
}

int amx_mlp_head_forward(const float* d_x, int n, int cin, int width, int n_layers, const float* const* w,
                         const float* const* gamma, const float* const* beta, float* const* running_mean,
                         float* const* running_var, float eps, float momentum, int act, float slope, float* d_z, float* d_y,
                         float* d_mean, float* d_rstd, void* stream) {
  if (!d_x || !w || !gamma || !beta || !running_mean || !running_var || !d_z || !d_y || !d_mean || !d_rstd)
    return fail(AMX_ERR_INVALID, "null argument");
  if (int rc = mlp_check(n, cin, width, n_layers)) return rc;
  if (act != AMX_ACT_NONE && act != AMX_ACT_RELU && act != AMX_ACT_LRELU) return fail(AMX_ERR_INVALID, "unsupported activation");
  const size_t plane = (size_t)n * width;
  for (int l = 0; l < n_layers; ++l) {
    if (!w[l] || (!gamma[l] != !beta[l]) || (!running_mean[l] != !running_var[l])) return fail(AMX_ERR_INVALID, "layer %d: bad parameter pointers", l);
    AMX_HIP(amx::launch_mlp_layer_forward(l ? d_y + (l - 1) * plane : d_x, n, l ? width : cin, w[l], width, gamma[l], beta[l], eps,
                                          l + 1 < n_layers ? act : AMX_ACT_NONE, slope, d_z + l * plane, d_y + l * plane,
                                          d_mean + (size_t)l * width, d_rstd + (size_t)l * width, running_mean[l], running_var[l],
                                          momentum, (hipStream_t)stream));
  }
  return AMX_OK;
}

size_t amx_mlp_head_scratch_bytes(int n, int cin, int width) { return amx::mlp_backward_scratch_floats(n, cin, width) * sizeof(float); }

int amx_mlp_head_backward(const float* d_dy, const float* d_x, int n, int cin, int width, int n_layers,
                          const float* const* w, const float* const* gamma, int act, float slope, const float* d_z,
                          const float* d_y, const float* d_mean, const float* d_rstd, float* const* dw, float* const* dgamma,
                          float* const* dbeta, float* d_dx, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (!d_dy || !d_x || !w || !gamma || !d_z || !d_y || !d_mean || !d_rstd || !dw || !dgamma || !dbeta || !d_scratch)
    return fail(AMX_ERR_INVALID, "null argument");
  if (int rc = mlp_check(n, cin, width, n_layers)) return rc;
  if (int rc = amx::need_scratch(amx_mlp_head_scratch_bytes(n, cin, width), scratch_bytes)) return rc;
  const size_t plane = (size_t)n * width;
  float* dz = (float*)d_scratch;
  float* dprev = dz + plane;
  for (int l = n_layers - 1; l >= 0; --l) {
    if (!w[l] || !dw[l] || (gamma[l] && (!dgamma[l] || !dbeta[l]))) return fail(AMX_ERR_INVALID, "layer %d: bad parameter pointers", l);
    AMX_HIP(amx::launch_mlp_layer_backward(l + 1 < n_layers ? dprev : d_dy, d_y + l * plane, d_z + l * plane,
                                           d_mean + (size_t)l * width, d_rstd + (size_t)l * width, gamma[l],
                                           l + 1 < n_layers ? act : AMX_ACT_NONE, slope, l ? d_y + (l - 1) * plane : d_x, w[l], n,
                                           l ? width : cin, width, dz, gamma[l] ? dgamma[l] : nullptr, gamma[l] ? dbeta[l] : nullptr,
                                           dw[l], l ? dprev : d_dx, dprev + plane, (hipStream_t)stream));
  }
  return AMX_OK;
}

// ---- the heads / losses of ONE contrastive step as batches: n_heads chains of the same length run as one chain of launches
int amx_mlp_heads_forward(int n_heads, const float* const* d_x, int n, const int* cin, int width, int n_layers, const float* const* w,
                          const float* const* gamma, const float* const* beta, float* const* running_mean, float* const* running_var,
                          float eps, float momentum, int act, float slope, float* const* d_z, float* const* d_y, float* const* d_mean,
                          float* const* d_rstd, void* stream) {
  if (!d_x || !cin || !w || !gamma || !beta || !running_mean || !running_var || !d_z || !d_y || !d_mean || !d_rstd)
    return fail(AMX_ERR_INVALID, "null argument");
  if (n_heads < 1 || n_heads > amx::MLP_MAXB) return fail(AMX_ERR_INVALID, "1 <= heads <= %d (got %d)", amx::MLP_MAXB, n_heads);
  if (act != AMX_ACT_NONE && act != AMX_ACT_RELU && act != AMX_ACT_LRELU) return fail(AMX_ERR_INVALID, "unsupported activation");
  const size_t plane = (size_t)n * width;
  for (int h = 0; h < n_heads; ++h) {
    if (int rc = mlp_check(n, cin[h], width, n_layers)) return rc;
    if (!d_x[h] || !d_z[h] || !d_y[h] || !d_mean[h] || !d_rstd[h]) return fail(AMX_ERR_INVALID, "head %d: null buffer", h);
    for (int l = 0; l < n_layers; ++l) {
      const int i = h * n_layers + l;
      if (!w[i] || (!gamma[i] != !beta[i]) || (!running_mean[i] != !running_var[i]))
        return fail(AMX_ERR_INVALID, "head %d layer %d: bad parameter pointers", h, l);
    }
  }
  for (int l = 0; l < n_layers; ++l) {
    const float *x[amx::MLP_MAXB], *wl[amx::MLP_MAXB], *gl[amx::MLP_MAXB], *bl[amx::MLP_MAXB];
    float *z[amx::MLP_MAXB], *y[amx::MLP_MAXB], *mu[amx::MLP_MAXB], *rs[amx::MLP_MAXB], *rm[amx::MLP_MAXB], *rv[amx::MLP_MAXB];
    int k[amx::MLP_MAXB];
    for (int h = 0; h < n_heads; ++h) {
      const int i = h * n_layers + l;
      x[h] = l ? d_y[h] + (l - 1) * plane : d_x[h];
      k[h] = l ? width : cin[h];
      wl[h] = w[i]; gl[h] = gamma[i]; bl[h] = beta[i]; rm[h] = running_mean[i]; rv[h] = running_var[i];
      z[h] = d_z[h] + l * plane; y[h] = d_y[h] + l * plane; mu[h] = d_mean[h] + (size_t)l * width; rs[h] = d_rstd[h] + (size_t)l * width;
    }
    AMX_HIP(amx::launch_mlp_heads_layer_forward(n_heads, x, n, k, wl, width, gl, bl, eps, l + 1 < n_layers ? act : AMX_ACT_NONE, slope,
                                                z, y, mu, rs, rm, rv, momentum, (hipStream_t)stream));
  }
  return AMX_OK;
}

int amx_mlp_heads_backward(int n_heads, const float* const* d_dy, const float* const* d_x, int n, const int* cin, int width, int n_layers,
                           const float* const* w, const float* const* gamma, int act, float slope, const float* const* d_z,
                           const float* const* d_y, const float* const* d_mean, const float* const* d_rstd, float* const* dw,
                           float* const* dgamma, float* const* dbeta, float* const* d_dx, void* const* d_scratch, size_t scratch_bytes,
                           void* stream) {
  if (!d_dy || !d_x || !cin || !w || !gamma || !d_z || !d_y || !d_mean || !d_rstd || !dw || !dgamma || !dbeta || !d_dx || !d_scratch)
    return fail(AMX_ERR_INVALID, "null argument");
  if (n_heads < 1 || n_heads > amx::MLP_MAXB) return fail(AMX_ERR_INVALID, "1 <= heads <= %d (got %d)", amx::MLP_MAXB, n_heads);
  const size_t plane = (size_t)n * width;
  for (int h = 0; h < n_heads; ++h) {
    if (int rc = mlp_check(n, cin[h], width, n_layers)) return rc;
    if (scratch_bytes < amx_mlp_head_scratch_bytes(n, cin[h], width))
      return fail(AMX_ERR_WORKSPACE, "head %d: scratch needs %zu bytes (got %zu)", h, amx_mlp_head_scratch_bytes(n, cin[h], width), scratch_bytes);
    if (!d_dy[h] || !d_x[h] || !d_z[h] || !d_y[h] || !d_mean[h] || !d_rstd[h] || !d_scratch[h]) return fail(AMX_ERR_INVALID, "head %d: null buffer", h);
    for (int l = 0; l < n_layers; ++l) {
      const int i = h * n_layers + l;
      if (!w[i] || !dw[i] || (gamma[i] && (!dgamma[i] || !dbeta[i]))) return fail(AMX_ERR_INVALID, "head %d layer %d: bad parameter pointers", h, l);
    }
  }
  for (int l = n_layers - 1; l >= 0; --l) {
    const float *dy[amx::MLP_MAXB], *y[amx::MLP_MAXB], *z[amx::MLP_MAXB], *mu[amx::MLP_MAXB], *rs[amx::MLP_MAXB], *gl[amx::MLP_MAXB];
    const float *x[amx::MLP_MAXB], *wl[amx::MLP_MAXB];
    float *dz[amx::MLP_MAXB], *dg[amx::MLP_MAXB], *db[amx::MLP_MAXB], *dwl[amx::MLP_MAXB], *dx[amx::MLP_MAXB], *wpart[amx::MLP_MAXB];
    int k[amx::MLP_MAXB];
    for (int h = 0; h < n_heads; ++h) {
      const int i = h * n_layers + l;
      float* dzb = (float*)d_scratch[h];
      float* dprev = dzb + plane;
      dy[h] = l + 1 < n_layers ? dprev : d_dy[h];
      y[h] = d_y[h] + l * plane; z[h] = d_z[h] + l * plane; mu[h] = d_mean[h] + (size_t)l * width; rs[h] = d_rstd[h] + (size_t)l * width;
      gl[h] = gamma[i]; x[h] = l ? d_y[h] + (l - 1) * plane : d_x[h]; wl[h] = w[i]; k[h] = l ? width : cin[h];
      dz[h] = dzb; dg[h] = gamma[i] ? dgamma[i] : nullptr; db[h] = gamma[i] ? dbeta[i] : nullptr; dwl[h] = dw[i];
      dx[h] = l ? dprev : d_dx[h]; wpart[h] = dprev + plane;
    }
    AMX_HIP(amx::launch_mlp_heads_layer_backward(n_heads, dy, y, z, mu, rs, gl, l + 1 < n_layers ? act : AMX_ACT_NONE, slope, x, wl, n, k,
                                                 width, dz, dg, db, dwl, dx, wpart, (hipStream_t)stream));
  }
  return AMX_OK;
}

int amx_supcon_loss_batch(int n_losses, const float* const* d_feat, const int* const* d_labels, int n, int c, float temperature,
                          int weigh_rarity, int balance_denominator, int sqrt_mode, float* const* d_loss, float* const* d_grad,
                          void* d_scratch, size_t scratch_bytes, void* stream) {
  if (!d_feat || !d_labels || !d_loss || !d_scratch) return fail(AMX_ERR_INVALID, "null argument");
  if (n_losses < 1 || n_losses > amx::MLP_MAXB) return fail(AMX_ERR_INVALID, "1 <= losses <= %d (got %d)", amx::MLP_MAXB, n_losses);
  if (n < 2 || n > 16384 || c < 1 || !(temperature > 0.f)) return fail(AMX_ERR_INVALID, "bad sizes (n=%d c=%d T=%g)", n, c, temperature);
  if (int rc = amx::need_scratch(n_losses * amx::supcon_scratch_bytes(n, c), scratch_bytes)) return rc;
  for (int b = 0; b < n_losses; ++b) {
    if (!d_feat[b] || !d_labels[b] || !d_loss[b]) return fail(AMX_ERR_INVALID, "loss %d: null buffer", b);
    if (d_grad && (!d_grad[b] != !d_grad[0])) return fail(AMX_ERR_INVALID, "gradients for all losses or for none");
  }
  AMX_HIP(amx::launch_supcon_batch(n_losses, d_feat, d_labels, n, c, temperature, weigh_rarity, balance_denominator, sqrt_mode, d_loss,
                                   d_grad, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

int amx_gather_labels_batch(const float* d_seg, int sd, int sh, int sw, int n_maps, const long long* const* d_coords, int p, const int* dims,
                            int views, int* const* d_labels, void* stream) {
  if (!d_seg || !d_coords || !dims || !d_labels || p < 1 || views < 1) return fail(AMX_ERR_INVALID, "gather_labels: bad arguments");
  if (n_maps < 1 || n_maps > amx::MLP_MAXB) return fail(AMX_ERR_INVALID, "1 <= maps <= %d (got %d)", amx::MLP_MAXB, n_maps);
  if (sd < 1 || sh < 1 || sw < 1) return fail(AMX_ERR_SHAPE, "gather_labels: non-positive shape");
  for (int b = 0; b < n_maps; ++b)
    if (!d_coords[b] || !d_labels[b] || dims[3 * b] < 1 || dims[3 * b + 1] < 1 || dims[3 * b + 2] < 1)
      return fail(AMX_ERR_SHAPE, "gather_labels: map %d: bad arguments", b);
  AMX_HIP(amx::launch_gather_labels_batch(d_seg, sd, sh, sw, n_maps, d_coords, p, dims, views, d_labels, (hipStream_t)stream));
  return AMX_OK;
}

int amx_sample_coords(const long long* d_draws, int n_draws, int num, int d0, int d1, int d2, long long* d_coords, void* stream) {
  if (!d_draws || !d_coords) return fail(AMX_ERR_INVALID, "null argument");
  if (num < 1 || n_draws < num || n_draws > 4096) return fail(AMX_ERR_INVALID, "1 <= num <= n_draws <= 4096 (got %d, %d)", num, n_draws);
  if (d0 < 1 || d1 < 1 || d2 < 1) return fail(AMX_ERR_SHAPE, "non-positive shape");
  AMX_HIP(amx::launch_sample_coords(d_draws, n_draws, num, d0, d1, d2, d_coords, (hipStream_t)stream));
  return AMX_OK;
}

int amx_import_input(const float* d_src, void* d_dst, int n, int cin, int d, int hh, int w, int precision, void* stream) {
  if (!d_src || !d_dst || n < 1 || d < 1 || hh < 1 || w < 1) return fail(AMX_ERR_INVALID, "import_input: bad arguments");
  if (cin < 1 || cin > 16) return fail(AMX_ERR_SHAPE, "import_input: 1 <= input channels <= 16 (got %d)", cin);
  if (precision != AMX_PREC_F16 && precision != AMX_PREC_BF16) return fail(AMX_ERR_INVALID, "import_input: f16 / bf16 storage");
  AMX_HIP(amx::launch_import_input(d_src, d_dst, n, cin, (long long)d * hh * w, precision, (hipStream_t)stream));
  return AMX_OK;
}

int amx_gather_labels(const float* d_seg, int sd, int sh, int sw, const long long* d_coords, int p, int d, int hh, int w, int views,
                      int* d_labels, void* stream) {
  if (!d_seg || !d_coords || !d_labels || p < 1 || views < 1) return fail(AMX_ERR_INVALID, "gather_labels: bad arguments");
  if (sd < 1 || sh < 1 || sw < 1 || d < 1 || hh < 1 || w < 1) return fail(AMX_ERR_SHAPE, "gather_labels: non-positive shape");
  AMX_HIP(amx::launch_gather_labels(d_seg, sd, sh, sw, d_coords, p, d, hh, w, views, d_labels, (hipStream_t)stream));
  return AMX_OK;
}

int amx_sample_perm(const long long* d_keys, int d0, int d1, int d2, int num, long long* d_coords, void* stream) {
  if (!d_keys || !d_coords) return fail(AMX_ERR_INVALID, "null argument");
  if (d0 < 1 || d1 < 1 || d2 < 1) return fail(AMX_ERR_SHAPE, "non-positive shape");
  const long long nvox = (long long)d0 * d1 * d2;
  if (nvox > 4096 || num < 1 || num > nvox) return fail(AMX_ERR_INVALID, "sample_perm: 1 <= num <= d0 d1 d2 <= 4096 (got %d of %lld)", num, nvox);
  AMX_HIP(amx::launch_sample_perm(d_keys, (int)nvox, num, d1, d2, d_coords, (hipStream_t)stream));
  return AMX_OK;
}

int amx_gather_rows(const void* d_src, int dtype, long long src_sn, long long src_sz, long long src_sy, long long src_sx, long long src_sc,
                    const long long* d_coords, int n, int p, int c, float* d_rows, void* stream) {
  if (!d_src || !d_coords || !d_rows || n < 1 || p < 1 || c < 1 || dtype < 0 || dtype > 2) return fail(AMX_ERR_INVALID, "gather_rows: bad arguments");
  AMX_HIP(amx::launch_gather_rows(d_src, dtype, src_sn, src_sz, src_sy, src_sx, src_sc, d_coords, n, p, c, d_rows, (hipStream_t)stream));
  return AMX_OK;
}

int amx_scatter_rows(const float* d_rows, const long long* d_coords, void* d_dst, int precision, long long dst_sn, long long dst_sz,
                     long long dst_sy, long long dst_sx, int n, int p, int c, int accumulate, void* stream) {
  if (!d_rows || !d_coords || !d_dst || n < 1 || p < 1 || c < 1 || (precision != AMX_PREC_F16 && precision != AMX_PREC_BF16))
    return fail(AMX_ERR_INVALID, "scatter_rows: bad arguments");
  AMX_HIP(amx::launch_scatter_rows(d_rows, d_coords, d_dst, precision, dst_sn, dst_sz, dst_sy, dst_sx, n, p, c, accumulate, (hipStream_t)stream));
  return AMX_OK;
}

size_t amx_conv3d_backward_sampled_scratch_bytes(int p) { return amx::sampled_conv_backward_scratch_bytes(p); }

int amx_conv3d_backward_sampled(const float* d_grows, const long long* d_coords, const void* d_x, int x_channels, const float* d_w, int n,
                                int p, int d, int hh, int w, int cout, int cin, float* d_dw, void* d_din, int din_channels, void* d_scratch,
                                size_t scratch_bytes, int precision, void* stream) {
  if (!d_scratch || scratch_bytes < amx::sampled_conv_backward_scratch_bytes(p))
    return fail(AMX_ERR_WORKSPACE, "conv3d_backward_sampled: scratch needs %zu bytes", amx::sampled_conv_backward_scratch_bytes(p));
  if (!d_grows || !d_coords || !d_x || !d_w || !d_dw || n < 1 || p < 1) return fail(AMX_ERR_INVALID, "conv3d_backward_sampled: bad arguments");
  if (precision != AMX_PREC_F16 && precision != AMX_PREC_BF16) return fail(AMX_ERR_INVALID, "conv3d_backward_sampled: f16 / bf16 storage");
  if (cout < 1 || cout > 16 || cin < 1 || cin > 16 || x_channels < cin || (d_din && din_channels < cin))
    return fail(AMX_ERR_SHAPE, "conv3d_backward_sampled: 1 <= cout, cin <= 16 (got %d, %d)", cout, cin);
  if (d < 2 || hh < 2 || w < 2 || p > 1024) return fail(AMX_ERR_SHAPE, "conv3d_backward_sampled: sizes >= 2, at most 1024 sampled voxels");
  AMX_HIP(amx::launch_sampled_conv_backward(d_grows, d_coords, d_x, x_channels, d_w, n, p, d, hh, w, cout, cin, d_dw, d_din, din_channels,
                                            d_scratch, precision, (hipStream_t)stream));
  return AMX_OK;
}

int amx_upsample2_trilinear_backward(const void* d_gout, void* d_gin, int n, int din, int hin, int win, int c, int precision,
                                     void* stream) {
  if (!d_gout || !d_gin || c % 8 || n < 1 || din < 1 || hin < 1 || win < 1) return fail(AMX_ERR_INVALID, "bad argument");
  AMX_HIP(amx::launch_upsample2_trilinear_backward(d_gout, d_gin, n, din, hin, win, c, precision, (hipStream_t)stream));
  return AMX_OK;
}

int amx_export_ncdhw(const void* d_src, int c, int n, int d, int hh, int w, float* d_out, int precision, void* stream) {
  if (!d_src || !d_out || c % 8 || c < 8 || n < 1 || d < 1 || hh < 1 || w < 1) return fail(AMX_ERR_INVALID, "bad argument");
  AMX_HIP(amx::launch_export_ncdhw(d_src, c, nullptr, 0, 0, n, d, hh, w, d_out, precision, (hipStream_t)stream));
  return AMX_OK;
}

int amx_import_ncdhw(const float* d_src, void* d_dst, int n, int c, int d, int hh, int w, long long dst_sn, long long dst_sz,
                     long long dst_sy, long long dst_sx, int accumulate, int precision, void* stream) {
  if (!d_src || !d_dst || c % 8 || c < 8 || n < 1 || d < 1 || hh < 1 || w < 1) return fail(AMX_ERR_INVALID, "bad argument");
  if (dst_sx < (long long)c * 2 || (dst_sx & 15) || (dst_sy & 15) || (dst_sz & 15) || (dst_sn & 15) || ((size_t)d_dst & 15))
    return fail(AMX_ERR_INVALID, "destination strides must be multiples of 16 bytes with a voxel pitch >= 2 * c");
  AMX_HIP(amx::launch_import_ncdhw(d_src, d_dst, n, c, d, hh, w, dst_sn, dst_sz, dst_sy, dst_sx, accumulate, precision,
                                   (hipStream_t)stream));
  return AMX_OK;
}

int amx_upcat_split_backward(const void* d_dcat, void* d_dskip, void* d_dlow, int n, int dlow, int hlow, int wlow, int c0, int c1,
                             int accumulate_skip, int precision, void* stream) {
  if (!d_dcat || (!d_dskip && c0 > 0) || !d_dlow || n < 1 || dlow < 1 || hlow < 1 || wlow < 1 || c0 < 0 || c1 < 8 || c0 % 8 || c1 % 8)
    return fail(AMX_ERR_INVALID, "bad argument");                       // c0 == 0: no skip part (the whole tensor is summed over children)
  AMX_HIP(amx::launch_upcat_split(d_dcat, d_dskip, d_dlow, n, dlow, hlow, wlow, c0, c1, accumulate_skip, 0, precision,
                                  (hipStream_t)stream));
  return AMX_OK;
}

int amx_upcat_split_backward_framed(const void* d_g_framed, void* d_dskip, void* d_dlow, int n, int dlow, int hlow, int wlow, int c0,
                                    int c1, int accumulate_skip, int precision, void* stream) {
  if (!d_g_framed || (!d_dskip && c0 > 0) || !d_dlow || n < 1 || dlow < 1 || hlow < 1 || wlow < 1 || c0 < 0 || c1 < 8 || c0 % 8 || c1 % 8)
    return fail(AMX_ERR_INVALID, "bad argument");                       // c0 == 0: no skip part (the whole tensor is summed over children)
  AMX_HIP(amx::launch_upcat_split(d_g_framed, d_dskip, d_dlow, n, dlow, hlow, wlow, c0, c1, accumulate_skip, 1, precision,
                                  (hipStream_t)stream));
  return AMX_OK;
}

}  // extern "C"
