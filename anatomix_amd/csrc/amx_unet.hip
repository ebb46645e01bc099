// anatomix_amd -- the UNet handle of the C ABI (include/anatomix_amd.h): layer plan, parameter folding / packing, the workspace
// layout and the launch schedule of one forward.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "amx_launch.h"

namespace {

using namespace amx;   // fail and the precision helpers; launchers are written amx:: at their calls

constexpr int kMaxDowns = 7;     // amx_unet_create refuses more; sizes the per-level arrays of a forward

enum Kind { K_CONV, K_NORM, K_ACT, K_POOL, K_UP, K_FINAL_ACT };

struct ConvLayer {
  int module_idx = 0, cin = 0, cout = 0, norm_idx = -1;
  bool has_act = false, is_final = false;
  int level = 0;          // resolution level the conv runs at (0 = full)
  int q = 1;              // MFMA tiles per workgroup the weights are packed for
  int cin_pad = 0;        // STORED input channels: every segment padded to a multiple of 16 (ngf = 24: 24 -> 32)
  int cout_p = 0;         // stored output channels (cout rounded up to 16; the extra channels are exact zeros)
  int c0_real = 0, c0_p = 0;   // first conv of a decoder block: real / stored channels of the skip segment
  void* wpk = nullptr;    // packed A fragments
  void* wpk_up = nullptr; // second packing for the 16+32 -> 16 merged-tap kernel (amx_conv3d_upcat.hip)
  bool after_up = false;  // first conv of a decoder block: its input is cat(skip [cout channels], upsample(low [cin - cout]))
  void* wpk_skip = nullptr;   // wider concat layers, nearest upsample: 27-tap packing of the skip channels only ...
  void* wpk_merge = nullptr;  // ... and the merged-tap packing of the upsampled channels (amx_conv3d_upmerge.hip)
  float* in_gamma = nullptr;  // InstanceNorm3d(affine=True) weight / bias of the norm that follows (else null)
  float* in_beta = nullptr;
  float* scale = nullptr; // folded norm gain (applied to the weights at pack time)
  float* shift = nullptr; // epilogue bias
  // eval-BatchNorm layers only: UNFOLDED weights + the norm's own shift, for forwards that tap the pre-norm output
  void* wpk_raw = nullptr;
  int* mxs = nullptr;     // AMX_PREC_F16X2_MX: {E8M0 block-scale word of the fp8 weights, scratch for their maximum}
  void* wx = nullptr;     // AMX_PREC_F16X2_MX, 32 -> 32 layers: fp8 fragments of the normalise-on-load z-march kernel (amx_conv3d_zx.hip)
  bool raw_has_bias = false;  // conv bias under BatchNorm (the reference never builds that: use_bias == (norm=='instance'))
  bool loaded = false;
};

}  // namespace

struct amx_unet {
  amx_unet_cfg cfg;
  std::vector<int> kinds;
  std::vector<ConvLayer> convs;
  std::vector<int> encoder_idx, decoder_idx;
  std::vector<int> mod_c, mod_level;  // per module: channels / resolution level of `feat` after it (post-concat for Upsample)
  int pack_w = 0;  // spatial W the packing heuristic assumed (reference window: 128)
  // device flags raised by any epilogue that was about to store a value outside the f16 range (or NaN): a ring of kFlagSlots,
  // ONE PER FORWARD.  A forward clears its slot on its own stream before its first kernel and its last kernel mirrors the slot
  // into the (sticky) host flag -- so forwards of one handle that overlap on different streams (chunks in flight, pipelined window
  // batches) neither erase nor inherit each other's flag, and nothing is ever reset from another stream.
  static constexpr int kFlagSlots = 16;
  int* d_flags = nullptr;
  int* d_flag = nullptr;    // the slot of the forward being enqueued
  unsigned flag_next = 0;
  int* h_flag = nullptr;    // pinned host mirror, written by the last kernel of a forward when the device flag is up
  int* h_flag_dev = nullptr;   // the same memory as the device sees it
  hipEvent_t acc_done[2] = {nullptr, nullptr};   // amx_unet_forward_windows_pipelined: "slot s has finished accumulating"
  // amx_sliding_window: the stream that takes every other window batch (the caller's stream takes the rest), and the window weights
  amx::SwLanes sw_lanes;
  amx::SwMapCache sw_map;
};

namespace {

// Mirrors the list the reference constructor builds (anatomix/model/network.py:309-465): same
// module order, hence the same integer indices in state_dict keys and encoder/decoder ids.
void build_plan(amx_unet* h) {
  const amx_unet_cfg& c = h->cfg;
  const bool has_norm = c.norm != AMX_NORM_NONE, has_act = c.activation != AMX_ACT_NONE;
  auto add_block = [&](int cin, int cout, int level) {
    ConvLayer L;
    L.module_idx = (int)h->kinds.size();
    L.cin = cin;
    L.cout = cout;
    L.level = level;
    h->kinds.push_back(K_CONV);
    if (has_norm) {
      L.norm_idx = (int)h->kinds.size();
      h->kinds.push_back(K_NORM);
    }
    if (has_act) {
      L.has_act = true;
      h->kinds.push_back(K_ACT);
    }
    h->convs.push_back(L);
  };
  add_block(c.input_nc, c.ngf, 0);
  int in_ngf = c.ngf;
  for (int i = 0; i < c.num_downs; ++i) {
    const int mult = i == 0 ? 1 : 2;
    add_block(in_ngf, in_ngf * mult, i);
    if (c.doubleconv) add_block(in_ngf * mult, in_ngf * mult, i);
    h->encoder_idx.push_back((int)h->kinds.size() - 1);
    h->kinds.push_back(K_POOL);
    in_ngf *= mult;
  }
  add_block(in_ngf, in_ngf * 2, c.num_downs);
  if (c.doubleconv) add_block(in_ngf * 2, in_ngf * 2, c.num_downs);
  int mult = 1 << c.num_downs;
  for (int i = 0; i < c.num_downs; ++i) {
    h->decoder_idx.push_back((int)h->kinds.size());
    h->kinds.push_back(K_UP);
    const int m = c.use_skip ? mult + mult / 2 : mult;
    const int level = c.num_downs - 1 - i;
    add_block(c.ngf * m, c.ngf * (mult / 2), level);
    h->convs.back().after_up = c.use_skip != 0;
    if (c.use_skip) h->convs.back().c0_real = c.ngf * (mult / 2);
    if (c.doubleconv) add_block(c.ngf * (mult / 2), c.ngf * (mult / 2), level);
    mult /= 2;
  }
  ConvLayer F;
  F.module_idx = (int)h->kinds.size();
  F.cin = c.ngf * mult;
  F.cout = c.output_nc;
  F.level = 0;
  F.is_final = true;
  h->kinds.push_back(K_CONV);
  h->convs.push_back(F);
  if (c.final_act != AMX_ACT_NONE) h->kinds.push_back(K_FINAL_ACT);
  // channels / level of `feat` after every module, as Unet.forward sees it (network.py:479-502)
  int ch = c.input_nc, lvl = 0;
  size_t ci = 0;
  std::vector<int> skip_c;
  for (size_t i = 0; i < h->kinds.size(); ++i) {
    switch (h->kinds[i]) {
      case K_CONV: ch = h->convs[ci].cout; lvl = h->convs[ci].level; ++ci; break;
      case K_POOL: lvl += 1; break;
      case K_UP:
        lvl -= 1;
        if (c.use_skip) { ch += skip_c.back(); skip_c.pop_back(); }
        break;
      default: break;
    }
    for (int e : h->encoder_idx)
      if (e == (int)i && c.use_skip) skip_c.push_back(ch);
    h->mod_c.push_back(ch);
    h->mod_level.push_back(lvl);
  }
}

// widest tensor materialised at a level: its own width, or (trilinear) the upsampled image of the level below it
int level_channels(const amx_unet* h, int level) {
  const int own = ((h->cfg.ngf + 15) / 16 * 16) << level;      // stored width: ngf padded to 16 channels
  int c = (h->cfg.interp == AMX_INTERP_TRILINEAR && level < h->cfg.num_downs) ? 2 * own : own;
  // the output conv's result is staged in a level-0 slot when it leaves through the export pass (W < 32 or output_nc > 32):
  // output_nc may exceed ngf.  (Sizing this by ngf alone overran the slot for output_nc = 64 -- silent while the bytes behind
  // the workspace were unused, wrong results / faults once the allocator had neighbours there.)
  if (level == 0 && (h->cfg.output_nc + 15) / 16 * 16 > c) c = (h->cfg.output_nc + 15) / 16 * 16;
  return c;
}

struct Profiler {
  std::vector<hipEvent_t> ev;
  std::vector<amx_launch_record> rec;
  hipStream_t st;
  int mark(const amx_launch_record& r) {   // call BEFORE the launch it describes
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess || hipEventRecord(e, st) != hipSuccess) return -1;
    ev.push_back(e);
    rec.push_back(r);
    return 0;
  }
};

inline bool f16_stored(int precision) { return precision == AMX_PREC_F16 || precision == AMX_PREC_F16X2 || precision == AMX_PREC_F16X2_MX; }
// kernels without an fp8 stage of their own (the single-channel stem: its operand is the fp32 input) run their f16x2 variant
inline int stem_precision(int precision) { return is_mx(precision) ? AMX_PREC_F16X2 : precision; }

size_t level_bytes(const amx_unet* h, int level, int n, int d, int hh, int w) {
  const size_t vox = (size_t)(d >> level) * (hh >> level) * (w >> level);
  return align_up((size_t)n * vox * level_channels(h, level) * (size_t)elem_bytes(h->cfg.precision), 256);
}

// InstanceNorm scratch of a forward: the separate statistics pass needs 65536 entries per sample; a conv epilogue that writes the
// partial sums itself needs one slot per (brick, wave) of that layer
// (a, b) pairs of a norm whose apply pass is left to the consuming conv (f16x2mx, amx_conv3d_zx.hip): two buffers, used alternately,
// behind the statistics scratch -- the consumer writes ITS statistics into that scratch while it still reads its input's pairs
inline size_t kPendingAbBytes(int n) { return (size_t)n * 2048 * 2 * sizeof(float); }
size_t in_scratch_bytes(const amx_unet* h, int n, int d, int hh, int w) {
  long long worst = 0;
  if (h->cfg.norm == AMX_NORM_INSTANCE || h->cfg.norm == AMX_NORM_INSTANCE_AFFINE)
    for (const ConvLayer& L : h->convs) {
      if (L.norm_idx < 0) continue;
      const long long s = (long long)amx::conv_v2_stats_slots(d >> L.level, hh >> L.level, w >> L.level, L.q) * L.cout_p;
      worst = s > worst ? s : worst;
    }
  return align_up(amx::instnorm_scratch_bytes(n, h->cfg.ngf << h->cfg.num_downs, worst), 256) + 2 * kPendingAbBytes(n);
}

// fp32 partial tensors of the layers that split K across workgroups (conv3d_k3_ks, the deepest levels): the largest one
size_t ks_scratch_bytes(const amx_unet* h, int n, int d, int hh, int w) {
  size_t worst = 0;
  for (const ConvLayer& L : h->convs) {
    if (L.after_up || L.is_final || L.level == 0) continue;
    const size_t b = amx::conv_ks_part_bytes(L.cin_pad, L.cout_p, n, d >> L.level, hh >> L.level, w >> L.level, h->cfg.precision, L.q);
    worst = b > worst ? b : worst;
  }
  return align_up(worst, 256);
}

int check_shape(const amx_unet* h, int n, int d, int hh, int w) {
  const int L = h->cfg.num_downs;
  if (n < 1 || d < 1 || hh < 1 || w < 1) return fail(AMX_ERR_SHAPE, "non-positive shape");
  const int m = 1 << L;
  if (d % m || hh % m || w % m)
    return fail(AMX_ERR_SHAPE, "spatial dims (%d,%d,%d) must be divisible by 2^num_downs = %d", d, hh, w, m);
  if ((d >> L) < 2 || (hh >> L) < 2 || (w >> L) < 2)
    return fail(AMX_ERR_SHAPE, "bottleneck would be smaller than 2 voxels: reflect padding undefined");
  return AMX_OK;
}

// Feature taps of Unet.forward(input, layers, encode_only) (network.py:475-529): module ids in ascending order,
// one fp32 NCDHW device buffer per id; `stop` >= 0 ends the forward after that module (encode_only).
struct TapReq {
  const int* modules;
  int n;
  float* const* out;
  int stop;
};

// Where the buffers of one forward lie in the caller's workspace, as byte offsets from its base: three slots per resolution level,
// the InstanceNorm scratch (partial sums, then the two pending-(a, b) buffers at its end), the split-K scratch.  The one statement of
// the size amx_unet_workspace_bytes reports and the forward checks.
struct Layout {
  size_t level[kMaxDowns + 1];        // bytes of ONE slot of that level
  size_t in_scratch, in_bytes;
  size_t ks_scratch, ks_bytes;
  size_t total;
};
Layout layout(const amx_unet* h, int n, int d, int hh, int w) {
  Layout l{};
  for (int lv = 0; lv <= h->cfg.num_downs; ++lv) {
    l.level[lv] = level_bytes(h, lv, n, d, hh, w);
    l.total += 3 * l.level[lv];
  }
  l.in_scratch = l.total;
  l.in_bytes = in_scratch_bytes(h, n, d, hh, w);
  l.total += l.in_bytes;
  l.ks_scratch = l.total;
  l.ks_bytes = ks_scratch_bytes(h, n, d, hh, w);
  l.total += l.ks_bytes;
  return l;
}

// The arguments of one forward.  x: fp32 single-channel input view (byte strides); y: fp32 planar output view (element strides).
// x_offs / y_offs (host arrays, element offsets, sliding-window mode): sample i reads its window at
// x + x_offs[i] and accumulates into y + y_offs[i].  Only the stem and the output conv see the volume, so those
// two run once per window (windows overlap: their accumulations must stay ordered on the stream); every layer
// in between runs on the whole batch of windows.
struct ForwardArgs {
  const float* x;
  long long xs_n, xs_z, xs_y;
  float* y;
  long long ys_n, ys_c, ys_z, ys_y;
  const float* wmap;
  int n, d, hh, w;
  void* ws;
  size_t ws_bytes;
  hipStream_t st;
  Profiler* prof = nullptr;
  const long long* x_offs = nullptr;
  const long long* y_offs = nullptr;
  const TapReq* taps = nullptr;
  // amx_unet_forward_windows_pipelined: the other slot's "has finished accumulating" event to wait for, and this slot's to record
  hipEvent_t acc_gate = nullptr, acc_done = nullptr;
};

// a dense [n][C][d][hh][w] input / output pair
ForwardArgs dense_args(const amx_unet* h, const float* d_x, float* d_y, int n, int d, int hh, int w, void* ws, size_t ws_bytes, void* stream) {
  const long long vox = (long long)d * hh * w;
  return ForwardArgs{d_x, vox * 4, (long long)hh * w * 4, (long long)w * 4, d_y, vox * h->cfg.output_nc, vox, (long long)hh * w, w,
                     nullptr, n, d, hh, w, ws, ws_bytes, (hipStream_t)stream};
}

// Row-planar storage (amx_common.h, layout FMT 2): every tensor of f16x2mx, whose 192-byte channels-last voxels left the LDS-DMA
// of the generic kernel at 11-15 B/clk/CU (profiles/r03_dma_stride_ubench.txt); the layout gained 28 % per layer at 128^3.
// MEASURED for the wide (>= 64-channel) tensors of the single 16-bit precisions and not kept: at 32^3 .. 8^3 a stage's time is
// weight streaming and latency, not the halo gather -- 64 -> 64 @32^3 45.9 -> 44.0 us, 128 -> 128 @16^3 27.6 -> 26.7, 8^3
// unchanged; 2743 -> 2772 volumes/s (+1 %, inside the box-to-box noise).
struct Tensor {                                   // C: stored channels per voxel, Cr: the reference's channel count
  int level = 0, slot = -1, C = 0, Cr = 0;
  const float* ab = nullptr;                      // non-null: the tensor is RAW, its norm + activation pending: y = act(a x + b)
  int ab_act = AMX_ACT_NONE;                      //   ... with this activation
};

// What a conv reads: the fp32 network input (in->slot < 0), cat(skip, upsample(in)), upsample(in) alone, or in
struct Sources {
  const Tensor* in;
  bool up, full_up;                               // read through a x2 upsample; ... which is materialised (trilinear) at the conv's resolution
  const Tensor* skip;                             // the skip connection in front of the upsampled channels (null: none)
};

// What one conv -> norm -> act group runs.  Forward::plan_conv decides all of it before the group takes a slot, marks a profiler event
// or launches; the driver (Forward::conv_group) and the parameter builders only read it.
enum class ConvKernel {
  Dispatch,      // amx::launch_conv, which picks z-march / split-K / generic by its own conv_route
  StemPair,      // the stem and the 16 -> 16 layer behind it as one launch (amx_conv3d_zmarch.hip, STEM)
  Stem,          // the fp32 single-channel input (amx_conv3d_stem.hip)
  Upcat16,       // 16 + up(32) -> 16 in one merged-tap launch (amx_conv3d_upcat.hip)
  Zx             // f16x2mx 32 -> 32, normalise-on-load z-march (amx_conv3d_zx.hip)
};
enum class ConvOut { Slot, Planar, SlotThenExport };   // a 16-bit slot; fp32 planar into y; a slot, then the export pass into y
enum class NormApply { Here, NextConv, Upsample, WithPool };   // who runs the apply pass of an instance norm (Forward::plan_norm)
struct ConvTerms {                                // what one launch reads and what its epilogue applies
  const void* wpk;
  const float* bias;
  int act;
};
struct ConvPlan {
  const ConvLayer* L;            // the group's conv
  const ConvLayer* Nx;           // StemPair: the 16 -> 16 layer, whose group this launch covers too (else null)
  Sources src;
  int lv, dd, dh, dw;            // level and extents the conv runs at
  size_t nxt;                    // module index of the next group
  ConvKernel kernel;
  bool merge;                    // merged taps: `first` covers the skip channels into a partial slot, amx::launch_conv_upmerge follows with `second`
  ConvTerms first, second;       // StemPair: the stem's and Nx's, applied by the one launch
  ConvOut out;
  bool inorm, act_on;            // an instance norm follows the conv; the group's activation runs (encode_only may end before it)
  bool raw_bn;                   // unfolded weights, pre-norm tap, then the folded BatchNorm as a pass of its own
  bool pool;                     // the epilogue also writes the max-pooled tensor
  bool stats;                    // the epilogue writes the InstanceNorm partial sums into the statistics scratch
  bool ks;                       // the split-K scratch is offered
  bool per_window;               // sliding windows: one launch per window, each at its own place in the volume
  float* tap_pre;                // exported from the stored RAW conv output, before the norm
  float* tap_post[3];            // exported from the finished tensor: the conv (no norm), norm and activation ids (in-place modules alias)
  float* tap_y;                  // the output conv: copied from y
};

// The launch schedule of one forward: the state that the modules hand to each other, and one method per step.
struct Forward : ForwardArgs {
  amx_unet* const h;
  const amx_unet_cfg& c;
  const bool split, mx;
  const long long eb;        // bytes per stored channel value (hi + lo halves in strict precision, + 2 of e4m3 copies)
  const int stop;            // encode_only: the module after which the forward ends (-1: none)

  char* slots[kMaxDowns + 1][3];   // activation arena: [level][slot]
  bool used[kMaxDowns + 1][3] = {};
  void* in_scratch = nullptr;
  float* ks_scratch = nullptr;
  size_t ks_bytes = 0;
  float* ab_buf[2] = {nullptr, nullptr};
  int ab_next = 0;

  size_t i = 0;              // module index
  size_t conv_i = 0;         // index of the next conv layer
  bool done = false;         // the module `stop` has run
  Tensor cur;                // current activation (slot -1: the fp32 network input)
  bool have_cur_up = false;  // cur is to be read through a x2 upsample by the next conv
  bool cur_is_full_up = false;   // cur is a materialised (trilinear) upsample at the consumer's resolution
  Tensor skips[kMaxDowns];
  int n_skips = 0;
  Tensor pend_skip;
  bool have_skip = false;
  Tensor fused_pool;         // pooled tensor written by the preceding conv's epilogue
  bool have_fused_pool = false;

  Forward(amx_unet* h_, const ForwardArgs& a)
      : ForwardArgs(a), h(h_), c(h_->cfg), split(is_split(c.precision)), mx(is_mx(c.precision)), eb(elem_bytes(c.precision)),
        stop(a.taps ? a.taps->stop : -1) {}

  // *s = a free slot of that level, now in use
  int slot(int level, int* s) {
    for (*s = 0; *s < 3; ++*s)
      if (!used[level][*s]) {
        used[level][*s] = true;
        return AMX_OK;
      }
    return fail(AMX_ERR_INVALID, "internal: arena exhausted at level %d", level);
  }
  char* mem(const Tensor& t) const { return t.slot < 0 ? nullptr : slots[t.level][t.slot]; }   // (no slot: the planar output conv's `out`)
  void release(const Tensor& t) { used[t.level][t.slot] = false; }
  // a tensor that was pushed as a skip connection stays alive until its decoder block has read it
  void release_unless_skip(const Tensor& t) {
    bool is_skip = false;
    for (int s = 0; s < n_skips; ++s)
      if (skips[s].level == t.level && skips[s].slot == t.slot) is_skip = true;
    if (!is_skip) release(t);
  }
  // encoder_idx marks the module AFTER which the skip is pushed (network.py:546-547)
  void push_skip_after(size_t module) {
    for (int e : h->encoder_idx)
      if (e == (int)module && c.use_skip) skips[n_skips++] = cur;
  }

  // module index behind the conv -> norm -> act group that starts at module `at`
  static size_t next_group(size_t at, const ConvLayer& L) { return at + 1 + (L.norm_idx >= 0 ? 1 : 0) + (L.has_act ? 1 : 0); }
  // f16x2mx: a tensor whose only reader is the convolution at module `nxt` needs no lo plane (convolutions read hi and the e4m3 copies);
  // feature taps read the pair, so any tap request keeps every plane
  int conv_only(size_t nxt) const { return mx && !taps && nxt < h->kinds.size() && h->kinds[nxt] == K_CONV; }

  float* tap_of(int module) const {
    if (taps)
      for (int t = 0; t < taps->n; ++t)
        if (taps->modules[t] == module) return taps->out[t];
    return nullptr;
  }
  // tap = fp32 NCDHW copy of a stored 16-bit tensor
  hipError_t export_slot(const Tensor& t, float* dst) {
    return amx::launch_export_ncdhw(mem(t), t.Cr, nullptr, 0, 0, n, d >> t.level, hh >> t.level, w >> t.level, dst, c.precision, st,
                                    t.C, 0);
  }
  // profiled forward: the record of the launch that follows (call BEFORE it), and the kernel name of the last record
  int record(int module_idx, int cin, int cout, int dd, int dh, int dw, double flops, double bytes) {
    if (!prof) return AMX_OK;
    amx_launch_record r;
    memset(&r, 0, sizeof r);
    r.module_idx = module_idx; r.cin = cin; r.cout = cout; r.n = n; r.d = dd; r.h = dh; r.w = dw;
    r.flops = flops; r.bytes = bytes;
    if (prof->mark(r)) return fail(AMX_ERR_HIP, "hipEventRecord failed");
    return AMX_OK;
  }
  void name_last(const char* fmt, ...) {
    if (!prof) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(prof->rec.back().kernel, sizeof prof->rec.back().kernel, fmt, ap);
    va_end(ap);
  }

  int run() {
    if (int e = check_shape(h, n, d, hh, w)) return e;
    for (const ConvLayer& L : h->convs)
      if (!L.loaded) return fail(AMX_ERR_NOT_LOADED, "conv model.%d has no parameters", L.module_idx);
    const Layout lay = layout(h, n, d, hh, w);
    if (ws_bytes < lay.total || ((uintptr_t)ws & 255))
      return fail(AMX_ERR_WORKSPACE, "workspace needs %zu bytes, 256-byte aligned (got %zu)", lay.total, ws_bytes);
    char* pcur = (char*)ws;
    for (int l = 0; l <= c.num_downs; ++l)
      for (int s = 0; s < 3; ++s) {
        slots[l][s] = pcur;
        pcur += lay.level[l];
      }
    in_scratch = (char*)ws + lay.in_scratch;                 // instance-norm partial sums + (a, b) pairs
    ab_buf[0] = (float*)((char*)in_scratch + lay.in_bytes - 2 * kPendingAbBytes(n));
    ab_buf[1] = (float*)((char*)in_scratch + lay.in_bytes - kPendingAbBytes(n));
    ks_bytes = lay.ks_bytes;
    ks_scratch = ks_bytes ? (float*)((char*)ws + lay.ks_scratch) : nullptr;
    if (c.input_nc > 1) {
      if (x_offs || wmap) return fail(AMX_ERR_INVALID, "the fused sliding-window path needs input_nc == 1");
      cur.level = 0; cur.C = 16; cur.Cr = c.input_nc;
      if (int e = slot(0, &cur.slot)) return e;
      AMX_HIP(amx::launch_import_input(x, mem(cur), n, c.input_nc, (long long)d * hh * w, c.precision, st));
    }
    for (i = 0; i < h->kinds.size() && !done; ++i) {
      int e = AMX_OK;
      switch (h->kinds[i]) {
        case K_CONV: e = conv_group(); break;
        case K_POOL: e = pool(); break;
        case K_UP: e = upsample(); break;
        case K_FINAL_ACT:      // fused into the last conv's epilogue; the caller's tensor at this id IS the network output
          if (float* t = tap_of((int)i))
            AMX_HIP(hipMemcpyAsync(t, y, (size_t)n * c.output_nc * d * hh * w * sizeof(float), hipMemcpyDeviceToDevice, st));
          break;
        default: break;      // K_NORM / K_ACT run inside their conv's group, which steps over them
      }
      if (e != AMX_OK) return e;
    }
    return AMX_OK;
  }

  Sources sources() const { return Sources{&cur, have_cur_up, cur_is_full_up, have_skip ? &pend_skip : nullptr}; }

  // ---- the plan of a group: what does not depend on the kernel.  Norm, activation and tap terms, the weights they call for, where the
  // output goes, and the refusals that follow from those
  int plan_terms(ConvPlan& pl) const {
    const ConvLayer& L = *pl.L;
    pl.inorm = L.norm_idx >= 0 && (c.norm == AMX_NORM_INSTANCE || c.norm == AMX_NORM_INSTANCE_AFFINE);
    if (pl.inorm && L.is_final) return fail(AMX_ERR_INVALID, "internal: instance norm after the output conv");
    // encode_only whose last layer is this group's conv / norm id: the modules after it never run in the reference,
    // so the (in-place) activation must not touch the tapped tensor
    const int idx_act = L.has_act ? L.module_idx + 1 + (L.norm_idx >= 0 ? 1 : 0) : -1;
    pl.act_on = L.has_act && !(stop >= L.module_idx && stop < idx_act);
    // ---- feature taps inside this conv -> norm -> act group.  The reference's activations are in-place modules
    // (network.py:188-196), so what the caller holds for a tap at the NORM id (or at the conv id when there is no
    // norm) is the activated tensor; only a conv followed by a norm yields a distinct, pre-norm tensor.
    float* const tap_conv = tap_of(L.module_idx);
    if (L.is_final) {
      pl.tap_y = tap_conv;   // contiguous [n][Cout][d][h][w] output (taps are only offered by the plain forward)
    } else {
      pl.tap_pre = L.norm_idx >= 0 ? tap_conv : nullptr;
      pl.tap_post[0] = L.norm_idx < 0 ? tap_conv : nullptr;
      pl.tap_post[1] = L.norm_idx >= 0 ? tap_of(L.norm_idx) : nullptr;
      pl.tap_post[2] = idx_act >= 0 ? tap_of(idx_act) : nullptr;
    }
    // pre-norm tap of a FOLDED eval-BatchNorm layer: run the conv with the unfolded weights, export, apply the norm
    pl.raw_bn = pl.tap_pre && !pl.inorm;
    if (pl.raw_bn && !L.wpk_raw) return fail(AMX_ERR_INVALID, "internal: model.%d has no unfolded packing", L.module_idx);
    if (pl.raw_bn && L.raw_has_bias)
      return fail(AMX_ERR_INVALID, "pre-norm tap of model.%d: conv bias under BatchNorm is not supported", L.module_idx);
    // InstanceNorm needs the whole (n, c) plane of RAW conv outputs first: the conv stores un-activated values and
    // amx::launch_instnorm normalises + activates them in place afterwards.  raw_bn: s * conv + L.shift is the whole folded norm
    // (amx::launch_affine_act)
    pl.first = pl.raw_bn ? ConvTerms{L.wpk_raw, nullptr, AMX_ACT_NONE}
                         : ConvTerms{L.wpk, L.shift, (pl.act_on && !pl.inorm) ? c.activation : AMX_ACT_NONE};
    if (L.is_final && c.final_act != AMX_ACT_NONE && stop != L.module_idx) pl.first.act = c.final_act;
    // the fp32 planar epilogues need W >= 32 and <= 32 output channels; outside that the output conv stores 16-bit
    // channels-last like any other layer and one export pass produces the fp32 NCDHW tensor
    const bool planar_ok = pl.dw >= 32 && L.cout_p <= 32 && L.cout_p == L.cout;
    pl.out = !L.is_final ? ConvOut::Slot : planar_ok ? ConvOut::Planar : ConvOut::SlotThenExport;
    if (pl.out == ConvOut::SlotThenExport && (wmap || x_offs))
      return fail(AMX_ERR_SHAPE, "sliding-window accumulation needs roi width >= 32 and output_nc <= 32");
    if (pl.src.in->slot < 0 && (L.is_final || L.cout_p > 32))
      return fail(AMX_ERR_INVALID, "stem kernel supports ngf in {16, 32} and a following layer (ngf=%d)", L.cout);
    return AMX_OK;
  }

  // ---- stem + the 16 -> 16 layer behind it as ONE launch (amx_conv3d_zmarch.hip, STEM): the stem's output never reaches HBM.
  // Plain forward only: no taps, folded (or no) norm on both layers, nothing else reads the stem's tensor.
  // pl: the stem's plan so far (conv `ci` at module `at`).  True: pl is now the pair's, and covers the group of conv ci + 1 too.
  bool plan_stem_pair(size_t ci, size_t at, ConvPlan& pl) const {
    const ConvLayer& L = *pl.L;
    const bool candidate = pl.src.in->slot < 0 && !split && (!x_offs || n <= 16) && L.cout_p == 16 && L.cout == 16 && !L.is_final && ci + 1 < h->convs.size() &&
                           (!L.has_act || c.activation == AMX_ACT_RELU || c.activation == AMX_ACT_NONE) && !pl.inorm;
    if (!candidate) return false;
    const ConvLayer& Nx = h->convs[ci + 1];
    const size_t g0 = pl.nxt;                 // module index of the next group
    const size_t g1 = next_group(g0, Nx);     // ... and of the one after it
    bool ok = g0 < h->kinds.size() && h->kinds[g0] == K_CONV && Nx.level == 0 && !Nx.is_final && !Nx.after_up && Nx.cin_pad == 16 &&
              Nx.cout_p == 16 && Nx.cout == 16 && Nx.q == 1 && Nx.loaded;
    for (int e : h->encoder_idx)
      if (e >= (int)at && e < (int)g0) ok = false;                                    // the stem's tensor would be a skip connection
    if (taps) {   // feature taps: only behind the pair (its activated output is module g1 - 1); the stem's tensor is never stored
      for (int t = 0; t < taps->n; ++t)
        if (taps->modules[t] + 1 < (int)g1) ok = false;
      if (taps->stop >= 0 && taps->stop + 1 < (int)g1) ok = false;
    }
    if (!ok) return false;      // (from here on no tap and no stop lies inside the stem's group: its terms are the plain ones)
    ConvPlan pair = pl;
    pair.kernel = ConvKernel::StemPair;
    pair.Nx = &Nx;
    pair.nxt = g1;
    pair.second = ConvTerms{Nx.wpk, Nx.shift, Nx.has_act ? c.activation : AMX_ACT_NONE};
    pair.tap_post[0] = tap_of((int)g1 - 1);
    if (!amx::conv_zmarch_stem_eligible(pair_params(pair, nullptr), c.precision)) return false;
    pl = pair;
    return true;
  }

  // ---- the plan of the group of conv `ci`, whose conv is module `at` and reads `src`.  Takes no slot, marks no event, launches
  // nothing; every refusal of a group is made here.  Each eligibility question is asked of ONE probe: the layer's launch parameters
  // as its builder binds them, with the memory that is not taken yet left null and nothing fused.
  int plan_conv(size_t ci, size_t at, const Sources& src, ConvPlan& pl) const {
    const ConvLayer& L = h->convs[ci];
    pl = ConvPlan{};
    pl.L = &L; pl.src = src; pl.lv = L.level; pl.dd = d >> L.level; pl.dh = hh >> L.level; pl.dw = w >> L.level;
    pl.nxt = next_group(at, L);
    if (int e = plan_terms(pl)) return e;
    if (plan_stem_pair(ci, at, pl)) return AMX_OK;
    amx::ConvParams p;
    if (int e = layer_params(pl, nullptr, nullptr, p)) return e;
    const bool stem = src.in->slot < 0, concat = src.up && src.skip, direct = !stem && !src.up;
    if (stem)
      pl.kernel = ConvKernel::Stem;
    else if (!split && !pl.raw_bn && L.wpk_up && concat && amx::conv_upcat16_eligible(p))
      pl.kernel = ConvKernel::Upcat16;
    // f16x2mx 32 -> 32 at whole tiles: the normalise-on-load z-march kernel.  It is the ONLY consumer of a tensor whose norm was
    // left pending (plan_norm), and takes already-normalised inputs too.
    else if (mx && L.wx && direct && !x_offs && (pl.inorm || pl.out == ConvOut::Planar) && amx::conv_zx_shape_eligible(p))
      pl.kernel = ConvKernel::Zx;
    else
      pl.kernel = ConvKernel::Dispatch;
    if (src.in->ab && pl.kernel != ConvKernel::Zx)
      return fail(AMX_ERR_INVALID, "internal: model.%d got an input whose norm is pending but cannot run the fused kernel", L.module_idx);
    if (pl.kernel == ConvKernel::Upcat16) pl.first.wpk = L.wpk_up;
    // wider concat layers: the ordinary convolution over the skip channels first (raw partial sums into a free slot of this
    // level), then the merged-tap convolution over the upsampled channels, which adds them, the bias and the activation
    pl.merge = pl.kernel == ConvKernel::Dispatch && !pl.raw_bn && L.wpk_merge && concat && !src.full_up && !L.is_final && L.cout_p == L.cout &&
               p.C0 == L.cout && amx::conv_upmerge_eligible(p.C0, p.C1, L.cout, pl.dd, pl.dh, pl.dw, p.up_shift, split);
    if (pl.merge) {
      pl.second = ConvTerms{L.wpk_merge, pl.first.bias, pl.first.act};
      pl.first = ConvTerms{L.wpk_skip, nullptr, AMX_ACT_NONE};
    }
    // nn.MaxPool3d(2) right after this block (network.py:368): fuse it into the z-marching epilogue
    pl.pool = !L.is_final && !pl.inorm && !pl.raw_bn && pl.nxt < h->kinds.size() && h->kinds[pl.nxt] == K_POOL && c.pooling == AMX_POOL_MAX && direct &&
              (split ? amx::conv_zmarch_can_pool_split(p) : amx::conv_zmarch_can_pool(p)) && L.q == L.cout_p / 16;
    // InstanceNorm layers on the generic kernel (and on Zx): the conv epilogue writes the partial sums of the statistics pass itself
    // (the stem of the split precisions likewise: amx_conv3d_stem.hip)
    const int stem_slots = (stem && pl.inorm && !x_offs) ? amx::conv_stem_stats_slots(p, stem_precision(c.precision)) : 0;
    pl.stats = pl.inorm && !pl.merge && pl.kernel != ConvKernel::Upcat16 && !x_offs &&
               (stem ? stem_slots > 0 : (pl.kernel == ConvKernel::Zx || amx::conv_fuses_stats(p, c.precision, L.q)));
    pl.ks = ks_scratch && direct && !L.is_final && !pl.raw_bn && !pl.merge &&
            amx::conv_ks_part_bytes(p.C0, p.Cout, n, pl.dd, pl.dh, pl.dw, c.precision, L.q) <= ks_bytes;
    // only the stem and the output conv see the volume: those two run once per window
    pl.per_window = x_offs && (stem || L.is_final);
    return AMX_OK;
  }

  // ---- launch parameters, one builder per launch kind; what a builder returns is launched as it stands
  // the input segments of a conv at dd x dh x dw
  int bind_sources(amx::ConvParams& p, const ConvLayer& L, const Sources& s, int dd, int dh, int dw) const {
    if (s.in->slot < 0) {  // stem: fp32 single-channel input
      p.src0 = (const char*)x;
      p.s0n = xs_n; p.s0z = xs_z; p.s0y = xs_y; p.s0x = 4;
      p.C0 = 16; p.C1 = 0; p.src0_f32c1 = 1;
    } else if (s.up) {
      const Tensor& lo = *s.in;
      // nearest: `lo` is the half-resolution tensor, read through >> 1; trilinear: already materialised at this level
      const int lw = s.full_up ? dw : dw / 2, lh = s.full_up ? dh : dh / 2, ld = s.full_up ? dd : dd / 2;
      p.up_shift = s.full_up ? 0 : 1;
      if (s.skip) {
        amx::set_src0(p, mem(*s.skip), s.skip->C, dd, dh, dw, c.precision);
      } else {  // no skip connection: the whole input is the upsampled tensor
        p.src0 = mem(lo);  // unused segment of zero channels
        p.C0 = 0;
      }
      amx::set_src1(p, mem(lo), lo.C, ld, lh, lw, c.precision);
    } else {
      amx::set_src0(p, mem(*s.in), s.in->C, dd, dh, dw, c.precision);
      p.C1 = 0;
    }
    if (p.C0 + p.C1 != L.cin_pad)
      return fail(AMX_ERR_INVALID, "internal: conv model.%d expects %d channels, schedule has %d",
                  L.module_idx, L.cin_pad, p.C0 + p.C1);
    return AMX_OK;
  }

  // the layer's own launch (merged taps: its skip-channel half, `out` then being the partial slot).  out / pooled: the memory of the
  // 16-bit output and of the fused pool's, null where the plan has none -- and in plan_conv's probe
  int layer_params(const ConvPlan& pl, char* out, char* pooled, amx::ConvParams& p) const {
    const ConvLayer& L = *pl.L;
    memset(&p, 0, sizeof p);
    p.N = n; p.D = pl.dd; p.H = pl.dh; p.W = pl.dw; p.Cout = L.cout_p;
    if (int e = bind_sources(p, L, pl.src, pl.dd, pl.dh, pl.dw)) return e;
    p.wpk = (const char*)pl.first.wpk; p.bias = pl.first.bias; p.act = pl.first.act; p.slope = c.act_slope;
    p.mxs = L.mxs;
    p.oflow = h->d_flag;
    if (pl.out == ConvOut::Planar) {
      p.out32 = y;
      p.pn = ys_n; p.pc = ys_c; p.pz = ys_z; p.py = ys_y;
      p.wmap = wmap;
    } else {
      amx::set_out(p, out, L.cout_p, pl.dd, pl.dh, pl.dw, c.precision);
    }
    if (pl.pool) amx::set_out2(p, pooled, L.cout_p, pl.dd / 2, pl.dh / 2, pl.dw / 2, c.precision);
    if (pl.stats) p.stats = (float*)in_scratch;
    if (pl.ks) p.part = ks_scratch;
    if (pl.merge) { p.src1 = nullptr; p.C1 = 0; p.up_shift = 0; }      // the skip channels only
    return AMX_OK;
  }
  // the merged-tap launch behind `skip` (layer_params of the same plan): reads the partial sums that one wrote, same layout as `out`
  amx::UpmergeParams merge_params(const ConvPlan& pl, const amx::ConvParams& skip, char* out) const {
    amx::UpmergeParams u;
    memset(&u, 0, sizeof u);
    amx::set_src(u, mem(*pl.src.in), pl.src.in->C, pl.dd / 2, pl.dh / 2, pl.dw / 2, c.precision);
    u.N = n; u.LD = pl.dd / 2; u.LH = pl.dh / 2; u.LW = pl.dw / 2; u.Cout = pl.L->cout;
    u.wpk = (const char*)pl.second.wpk; u.bias = pl.second.bias; u.act = pl.second.act; u.slope = c.act_slope;
    u.part = skip.out; u.out = out; u.ocs = skip.ocs;
    u.oflow = h->d_flag;
    return u;
  }
  // the stem pair: the 16 -> 16 layer's parameters (the stem's terms go to the launcher beside them); out null: plan_stem_pair's probe
  amx::ConvParams pair_params(const ConvPlan& pl, char* out) const {
    const ConvLayer& Nx = *pl.Nx;
    amx::ConvParams p;
    memset(&p, 0, sizeof p);
    p.N = n; p.D = pl.dd; p.H = pl.dh; p.W = pl.dw; p.Cout = Nx.cout_p; p.C0 = 16; p.C1 = 0;
    p.wpk = (const char*)pl.second.wpk; p.bias = pl.second.bias; p.act = pl.second.act; p.slope = c.act_slope;
    p.oflow = h->d_flag;
    amx::set_out(p, out, Nx.cout_p, pl.dd, pl.dh, pl.dw, c.precision);
    return p;
  }
  // window wi of a per-window launch: the stem reads its window of the volume, the output conv accumulates into its window of y
  amx::ConvParams window_params(const amx::ConvParams& p, int wi) const {
    amx::ConvParams q = p;
    q.N = 1;
    if (p.src0_f32c1) {
      q.src0 = (const char*)(x + x_offs[wi]);
      q.out = p.out + (long long)wi * p.on;
      if (p.out2) q.out2 = p.out2 + (long long)wi * p.qn;
    } else {
      q.src0 = p.src0 + (long long)wi * p.s0n;
      if (p.src1) q.src1 = p.src1 + (long long)wi * p.s1n;
      q.out32 = y + y_offs[wi];
    }
    return q;
  }

  // ---- the launches of a group
  hipError_t launch_one(const ConvPlan& pl, const amx::ConvParams& q, amx::ConvLaunchInfo* want) {
    switch (pl.kernel) {
      case ConvKernel::StemPair:
        return amx::launch_conv_zmarch_stem(q, x, xs_n, xs_z, xs_y, x_offs, pl.first.wpk, pl.first.bias, pl.first.act, c.act_slope, c.precision, st, want);
      case ConvKernel::Stem: return amx::launch_conv_stem(q, stem_precision(c.precision), st, want);
      case ConvKernel::Upcat16: return amx::launch_conv_upcat16(q, c.precision, st, want);
      case ConvKernel::Zx: return amx::launch_conv_zx(q, pl.src.in->ab, pl.src.in->ab_act, c.act_slope, pl.L->wx, st, want);
      case ConvKernel::Dispatch: break;
    }
    return amx::launch_conv(q, c.precision, pl.L->q, st, want);
  }
  // one launch, or one per window between the two event gates; then the merged-tap launch.  info: what the (last) launch ran and the
  // statistics slots it wrote, for the record and for the norm behind it
  int launch_group(const ConvPlan& pl, const Tensor& out, const Tensor& part, amx::ConvLaunchInfo& info) {
    amx::ConvParams p;
    if (pl.kernel == ConvKernel::StemPair)
      p = pair_params(pl, mem(out));
    else if (int e = layer_params(pl, mem(pl.merge ? part : out), pl.pool ? mem(fused_pool) : nullptr, p))
      return e;
    amx::ConvLaunchInfo* const want = (prof || pl.stats) ? &info : nullptr;
    // pipelined windows (two batches in flight on two streams): the accumulating launches of this batch wait for the other
    // slot's accumulations, so that overlapping windows still add up in window order
    const bool accumulates = x_offs && pl.L->is_final;
    if (accumulates && acc_gate) AMX_HIP(hipStreamWaitEvent(st, acc_gate, 0));
    if (pl.per_window) {
      for (int wi = 0; wi < n; ++wi) AMX_HIP(launch_one(pl, window_params(p, wi), want));
    } else {
      AMX_HIP(launch_one(pl, p, want));
    }
    if (accumulates && acc_done) AMX_HIP(hipEventRecord(acc_done, st));
    if (pl.merge) {
      amx::ConvLaunchInfo merge_info;
      AMX_HIP(amx::launch_conv_upmerge(merge_params(pl, p, mem(out)), c.precision, st, prof ? &merge_info : nullptr));
      if (prof) name_last("%.34s + %.26s", info.name, merge_info.name + 7);      // (+ 7: without its "conv3d_")
    } else if (prof) {
      name_last("%s", info.name);
    }
    return AMX_OK;
  }

  // the profiler record of the group's conv (call BEFORE its launch)
  int record_group(const ConvPlan& pl) {
    const ConvLayer& L = *pl.L;
    const double vox = (double)n * pl.dd * pl.dh * pl.dw;
    if (pl.Nx) {
      const double macs = L.cin * L.cout + pl.Nx->cin * pl.Nx->cout;
      return record(L.module_idx, L.cin, pl.Nx->cout, pl.dd, pl.dh, pl.dw, 2.0 * 27.0 * macs * vox,
                    4.0 * vox + 2.0 * pl.Nx->cout * vox + 2.0 * 27.0 * macs);   // fp32 input once, 16-bit output once
    }
    // ALGORITHMIC bytes: 16-bit activations read once and written once + the weights, the upsampled
    // segment counted at its LOW resolution for either interpolation (a materialised trilinear tensor and the hi / lo / e4m3
    // planes of the split precisions are this build's storage choices, not the layer's traffic requirement)
    const Sources& s = pl.src;
    const int C0 = s.up ? (s.skip ? s.skip->C : 0) : s.in->C, C1 = s.up ? s.in->C : 0;
    const double in_b = s.in->slot < 0 ? 4.0 * vox : (C0 * vox + C1 * vox / 8.0) * 2.0;
    const double out_b = L.is_final ? 4.0 * L.cout * vox : 2.0 * L.cout * vox;
    return record(L.module_idx, L.cin, L.cout, pl.dd, pl.dh, pl.dw, 2.0 * 27.0 * L.cin * L.cout * vox, in_b + out_b + 2.0 * 27.0 * L.cin * L.cout);
  }

  // ---- one conv -> norm -> act group (the stem pair: two): plan; take slots; launch; then norm, taps, releases and bookkeeping
  int conv_group() {
    ConvPlan pl;
    if (int e = plan_conv(conv_i, i, sources(), pl)) return e;
    conv_i += pl.Nx ? 2 : 1;
    const ConvLayer& O = pl.Nx ? *pl.Nx : *pl.L;      // the layer whose output the group stores
    Tensor out, part;
    out.level = part.level = pl.lv; out.C = O.cout_p; out.Cr = O.cout;
    if (pl.out != ConvOut::Planar)
      if (int e = slot(pl.lv, &out.slot)) return e;
    if (pl.pool) {
      fused_pool.level = pl.lv + 1; fused_pool.C = O.cout_p; fused_pool.Cr = O.cout;
      if (int e = slot(pl.lv + 1, &fused_pool.slot)) return e;
      have_fused_pool = true;
    }
    if (pl.merge)
      if (int e = slot(pl.lv, &part.slot)) return e;
    if (int e = record_group(pl)) return e;
    amx::ConvLaunchInfo info{};
    if (int e = launch_group(pl, out, part, info)) return e;
    if (pl.merge) release(part);                      // the partial sums are dead once their consumer is enqueued (stream order)
    if (int e = finish_group(pl, out, pl.stats ? info.stats_slots : 0)) return e;
    // inputs are dead once their consumer is enqueued (stream order)
    if (cur.slot >= 0) release(cur);
    if (have_skip) release(pend_skip);
    have_skip = false;
    have_cur_up = false;
    cur_is_full_up = false;
    cur = out;
    i = pl.nxt - 1;              // step over the fused norm / activation modules (the stem pair: over the second group too)
    push_skip_after(i);
    if (stop >= pl.L->module_idx && stop <= (int)i) done = true;   // encode_only: layers[-1] lies in this group
    return AMX_OK;
  }

  // what follows the conv's launch: the pre-norm tap, the norm, the export pass, the taps of the finished tensor
  int finish_group(const ConvPlan& pl, Tensor& out, int slots_written) {
    const ConvLayer& L = *pl.L;
    if (pl.tap_pre) AMX_HIP(export_slot(out, pl.tap_pre));     // the stored raw convolution output, before the norm below
    if (pl.raw_bn)
      AMX_HIP(amx::launch_affine_act(mem(out), L.scale, L.shift, n, (long long)pl.dd * pl.dh * pl.dw, L.cout_p,
                                     pl.act_on ? c.activation : AMX_ACT_NONE, c.act_slope, c.precision, st, h->d_flag));
    if (pl.inorm)
      if (int e = instance_norm_after(pl, out, slots_written)) return e;
    if (pl.out == ConvOut::SlotThenExport)
      AMX_HIP(amx::launch_export_ncdhw(mem(out), L.cout, nullptr, 0, 0, n, pl.dd, pl.dh, pl.dw, y, c.precision, st, L.cout_p, 0));
    if (pl.tap_y)
      AMX_HIP(hipMemcpyAsync(pl.tap_y, y, (size_t)n * L.cout * pl.dd * pl.dh * pl.dw * sizeof(float), hipMemcpyDeviceToDevice, st));
    for (float* t : pl.tap_post)
      if (t) AMX_HIP(export_slot(out, t));
    return AMX_OK;
  }

  // Who runs the apply pass of the instance norm behind the group's conv, whose raw output is `out`.  Anyone but this group only in a
  // plain forward whose activation runs: a tap or a window batch reads the finished tensor.
  NormApply plan_norm(const ConvPlan& pl, const Tensor& out) const {
    if (taps || x_offs || pl.act_on != pl.L->has_act || pl.nxt >= h->kinds.size()) return NormApply::Here;
    switch (h->kinds[pl.nxt]) {
      case K_CONV: {
        // the module after this group is a conv that runs the normalise-on-load kernel on this tensor (so the tensor is no skip
        // connection, no pool / upsample input): asked of that layer's own plan, reading `out` as it will.  (The output conv takes a
        // pending norm too: fp32 planar epilogue, no importance map, no activation of its own.)
        ConvPlan nx;
        if (!mx || conv_i >= h->convs.size() || plan_conv(conv_i, pl.nxt, Sources{&out, false, false, nullptr}, nx) != AMX_OK) return NormApply::Here;
        return nx.kernel == ConvKernel::Zx ? NormApply::NextConv : NormApply::Here;
      }
      case K_POOL:
        // f16x2mx, pool right after this group: the apply pass also writes the pooled tensor (amx_norm.hip in_apply_pool_kernel); the
        // in-place tensor then has no reader left but the decoder's convolution, which takes hi and the copies
        return mx && !have_fused_pool && amx::in_apply_pool_eligible(c.precision, pl.dd, pl.dh, pl.dw, pl.L->cout_p) ? NormApply::WithPool : NormApply::Here;
      case K_UP:   // trilinear upsample right after this group (decoder): the upsample pass normalises its eight inputs on the way in
        return c.interp == AMX_INTERP_TRILINEAR ? NormApply::Upsample : NormApply::Here;
      default: return NormApply::Here;
    }
  }

  // InstanceNorm behind a conv that stored its RAW output in `out`: statistics, then the apply pass where plan_norm puts it.
  // slots_written: the partial-statistics slots per sample that the conv's epilogue wrote (0: it wrote none, the statistics pass runs)
  int instance_norm_after(const ConvPlan& pl, Tensor& out, int slots_written) {
    const ConvLayer& L = *pl.L;
    const int dd = pl.dd, dh = pl.dh, dw = pl.dw, act = pl.act_on ? c.activation : AMX_ACT_NONE;
    if (int e = record(L.norm_idx, L.cout, L.cout, dd, dh, dw, 0.0, (double)eb * L.cout * (double)n * dd * dh * dw * 3.0)) return e;
    name_last("instnorm+act");
    const NormApply where = plan_norm(pl, out);
    float* const abo = where == NormApply::Here ? nullptr : ab_buf[ab_next];      // the (a, b) pairs, for whoever applies them
    AMX_HIP(amx::launch_instnorm(mem(out), L.in_gamma, L.in_beta, c.norm_eps, n, (long long)dd * dh * dw, L.cout_p, act, c.act_slope,
                                 in_scratch, c.precision, st, h->d_flag, slots_written, slots_written ? L.shift : nullptr, dw,
                                 conv_only(pl.nxt), where == NormApply::Here ? 1 : 0, abo));
    switch (where) {
      case NormApply::Here: break;
      case NormApply::WithPool:
        fused_pool.level = pl.lv + 1; fused_pool.C = L.cout_p; fused_pool.Cr = L.cout;
        if (int e = slot(pl.lv + 1, &fused_pool.slot)) return e;
        AMX_HIP(amx::launch_in_apply_pool(mem(out), abo, mem(fused_pool), n, dd, dh, dw, L.cout_p, act, c.act_slope,
                                          c.pooling == AMX_POOL_AVG, 1, conv_only(pl.nxt + 1), h->d_flag, st));
        have_fused_pool = true;
        name_last("instnorm+act+pool2<%s>", c.pooling == AMX_POOL_AVG ? "avg" : "max");
        break;
      case NormApply::NextConv:
      case NormApply::Upsample:      // the tensor stays RAW: its reader applies y = act(a x + b)
        out.ab = abo;
        out.ab_act = act;
        ab_next ^= 1;
        name_last("instnorm statistics only (apply fused into the next %s)", where == NormApply::Upsample ? "upsample" : "conv");
        break;
    }
    return AMX_OK;
  }

  int pool() {
    const int lv = cur.level + 1;
    Tensor out;
    if (have_fused_pool) {   // already produced by the previous conv's epilogue (or by its norm's apply pass)
      out = fused_pool;
      have_fused_pool = false;
    } else {
      out.level = lv; out.C = cur.C; out.Cr = cur.Cr;
      if (int e = slot(lv, &out.slot)) return e;
      if (int e = record((int)i, cur.C, cur.C, d >> lv, hh >> lv, w >> lv, 0.0,
                         (double)eb * cur.C * (double)n * (d >> lv) * (hh >> lv) * (w >> lv) * 9.0))
        return e;
      name_last("pool2<%s>", c.pooling == AMX_POOL_AVG ? "avg" : "max");
      AMX_HIP(amx::launch_pool2(mem(cur), mem(out), n, d >> lv, hh >> lv, w >> lv, cur.C, c.pooling == AMX_POOL_AVG, c.precision, st,
                                conv_only(i + 1)));
    }
    release_unless_skip(cur);
    cur = out;
    if (float* t = tap_of((int)i)) AMX_HIP(export_slot(cur, t));
    if (stop == (int)i) done = true;
    return AMX_OK;
  }

  int upsample() {
    if (c.interp == AMX_INTERP_TRILINEAR) {
      // nn.Upsample(2,'trilinear') is materialised (16-bit NDHWC at the finer level); the conv that follows
      // then reads two full-resolution segments (up_shift = 0)
      const int lv = cur.level - 1;
      Tensor up;
      up.level = lv; up.C = cur.C; up.Cr = cur.Cr;
      if (int e = slot(lv, &up.slot)) return e;
      if (int e = record((int)i, cur.C, cur.C, d >> lv, hh >> lv, w >> lv, 0.0,
                         (double)eb * cur.C * (double)n * (d >> lv) * (hh >> lv) * (w >> lv) * 1.125))
        return e;
      name_last("upsample2<trilinear>");
      AMX_HIP(amx::launch_upsample2_trilinear(mem(cur), mem(up), n, d >> cur.level, hh >> cur.level, w >> cur.level, cur.C, c.precision,
                                              st, conv_only(i + 1), cur.ab, cur.ab_act, c.act_slope, h->d_flag));
      release(cur);
      cur = up;
      cur_is_full_up = true;
    }
    have_cur_up = true;
    if (c.use_skip) {
      pend_skip = skips[--n_skips];
      have_skip = true;
    }
    if (float* t = tap_of((int)i)) {   // taken after torch.cat((skip, up), 1) -- network.py:500-502
      const int lv = cur_is_full_up ? cur.level : cur.level - 1;
      AMX_HIP(amx::launch_export_ncdhw(have_skip ? mem(pend_skip) : nullptr, have_skip ? pend_skip.Cr : 0, mem(cur), cur.Cr,
                                       cur_is_full_up ? 0 : 1, n, d >> lv, hh >> lv, w >> lv, t, c.precision, st,
                                       have_skip ? pend_skip.C : 0, cur.C));
    }
    if (stop == (int)i) done = true;
    return AMX_OK;
  }
};

// An f16 overflow (or a NaN) seen by an earlier forward of this handle is reported by the NEXT call; the forward that
// produced it has already had its output overwritten with NaN on the device (poison_if_flag).
int pending_numerics_error(amx_unet* h) {
  if (h->h_flag && *(volatile int*)h->h_flag) {
    *(volatile int*)h->h_flag = 0;      // the device slots are per forward and cleared by their own forwards
    return fail(AMX_ERR_OVERFLOW, "a previous forward of this network produced values outside the f16 range (or NaN) in %s storage; "
                "its output was overwritten with NaN.  Use precision bf16 or strict (bf16x2), which keep fp32's exponent range",
                h->cfg.precision == AMX_PREC_F16X2 ? "f16x2" : (is_mx(h->cfg.precision) ? "f16x2mx" : "f16"));
  }
  return AMX_OK;
}

int run_forward(amx_unet* h, const ForwardArgs& a) {
  if (int e = pending_numerics_error(h)) return e;
  const bool f16_store = f16_stored(h->cfg.precision);
  if (h->d_flags) {
    h->d_flag = h->d_flags + (h->flag_next++ % amx_unet::kFlagSlots);
    if (f16_store) AMX_HIP(hipMemsetAsync(h->d_flag, 0, sizeof(int), a.st));
  }
  const int rc = Forward(h, a).run();
  if (rc == AMX_OK && f16_store && h->d_flag) {
    // the output tensor (plain forward: dense [n][Cout][d][hh][w]; windows: the accumulation volume is the caller's, its
    // extent is not known here -- the flag and the status call cover that path) is poisoned when the flag is up
    const bool poison = !a.wmap && !a.x_offs && !(a.taps && a.taps->stop >= 0);
    AMX_HIP(amx::launch_poison_if_flag(h->d_flag, h->h_flag_dev, poison ? a.y : nullptr,
                                       poison ? (long long)a.n * h->cfg.output_nc * a.d * a.hh * a.w : 0, a.st));
    if (!h->h_flag_dev) AMX_HIP(hipMemcpyAsync(h->h_flag, h->d_flag, sizeof(int), hipMemcpyDeviceToHost, a.st));   // unmapped host memory
  }
  return rc;
}

}  // namespace

extern "C" {

int amx_unet_numerics_status(amx_unet_t* h, int synchronize, void* stream) {
  if (!h) return fail(AMX_ERR_INVALID, "null handle");
  if (synchronize) AMX_HIP(hipStreamSynchronize((hipStream_t)stream));
  return pending_numerics_error(h);
}

int amx_unet_create(amx_unet_t** out, const amx_unet_cfg* cfg) {
  if (!out || !cfg) return fail(AMX_ERR_INVALID, "null argument");
  *out = nullptr;
  // ngf = 8 mod 16 (the reference's default width 24, network.py:268): the ngf-wide tensors are stored with 16-channel padding
  if (cfg->num_downs < 1 || cfg->num_downs > kMaxDowns || cfg->ngf < 8 || cfg->ngf % 8 || (cfg->ngf + 15) / 16 * 16 > 32)
    return fail(AMX_ERR_INVALID, "ngf must be 8, 16, 24 or 32 (the stem kernel stores 16 or 32 channels) and 1 <= num_downs <= 7 (got ngf=%d "
                "num_downs=%d)", cfg->ngf, cfg->num_downs);
  // input_nc > 1: the input is imported into a 16-channel tensor and the first conv is an ordinary layer; output_nc that is not a
  // multiple of 16: the output conv stores padded channels and an export pass writes the fp32 NCDHW tensor
  if (cfg->input_nc < 1 || cfg->input_nc > 16) return fail(AMX_ERR_INVALID, "HIP path supports 1 <= input_nc <= 16 (got %d)", cfg->input_nc);
  if (cfg->output_nc < 1 || cfg->output_nc > 2048) return fail(AMX_ERR_INVALID, "output_nc out of range (got %d)", cfg->output_nc);
  if (cfg->norm < AMX_NORM_NONE || cfg->norm > AMX_NORM_INSTANCE_AFFINE)
    return fail(AMX_ERR_INVALID, "unknown norm mode %d", cfg->norm);
  if (cfg->interp != AMX_INTERP_NEAREST && cfg->interp != AMX_INTERP_TRILINEAR)
    return fail(AMX_ERR_INVALID, "unknown interp mode %d", cfg->interp);
  if ((cfg->ngf << cfg->num_downs) > 2048)
    return fail(AMX_ERR_INVALID, "widest layer has %d channels; the instance-norm kernels handle <= 2048", cfg->ngf << cfg->num_downs);
  if (cfg->activation < AMX_ACT_NONE || cfg->activation > AMX_ACT_LRELU || cfg->final_act < AMX_ACT_NONE ||
      cfg->final_act > AMX_ACT_LRELU)
    return fail(AMX_ERR_INVALID, "unsupported activation");
  if (cfg->precision < AMX_PREC_F16 || cfg->precision > AMX_PREC_F16X2_MX)
    return fail(AMX_ERR_INVALID, "unsupported precision %d", cfg->precision);
  // the fp8 correction stages exist in the generic kernel only; the consumers of a conv's output must be passes that write the e4m3
  // copies (norm apply, pool, upsample) -- i.e. networks that normalise with live statistics, the ones that need a strict mode at all
  if (is_mx(cfg->precision) && cfg->norm != AMX_NORM_INSTANCE && cfg->norm != AMX_NORM_INSTANCE_AFFINE)
    return fail(AMX_ERR_INVALID, "precision f16x2mx is implemented for the InstanceNorm configurations (norm='instance' / 'instance_affine'); "
                "use 'strict' (bf16x2) for this network");
  if (is_mx(cfg->precision) && cfg->input_nc != 1)
    return fail(AMX_ERR_INVALID, "precision f16x2mx needs input_nc == 1 (got %d)", cfg->input_nc);
  amx_unet* h = new amx_unet();
  h->cfg = *cfg;
  build_plan(h);
  h->pack_w = 128;
  for (ConvLayer& L : h->convs) {
    L.cout_p = (L.cout + 15) / 16 * 16;
    if (L.after_up && L.c0_real) {            // cat(skip, up): each segment padded on its own
      L.c0_p = (L.c0_real + 15) / 16 * 16;
      L.cin_pad = L.c0_p + (L.cin - L.c0_real + 15) / 16 * 16;
    } else {
      L.cin_pad = (L.cin + 15) / 16 * 16;
    }
    // Q is chosen for the reference operating point (128^3 windows): level l runs at W = 128>>l.
    const int w_at = h->pack_w >> L.level;
    L.q = amx::conv_pick_q(L.cout_p, w_at > 0 ? w_at : 1, cfg->precision);
    const size_t wbytes = (size_t)L.cout_p * L.cin_pad * 28 * 2 * (is_split(cfg->precision) ? 2 : 1);   // strict: [Wh | Wl]
    hipError_t e = hipMalloc(&L.wpk, wbytes);
    if (e == hipSuccess && !is_split(cfg->precision) && L.cin == 48 && L.cout == 16 && cfg->use_skip && cfg->interp == AMX_INTERP_NEAREST)
      e = hipMalloc(&L.wpk_up, amx::conv_upcat16_packed_bytes());
    // wider concat layers (nearest upsample): split into skip conv + merged-tap conv over the upsampled channels, at the levels
    // that are at least 32 voxels wide at the reference operating point
    if (e == hipSuccess && is_mx(cfg->precision)) e = hipMalloc((void**)&L.mxs, 2 * sizeof(int));
    if (e == hipSuccess && is_mx(cfg->precision) && L.cin_pad == 32 && L.cout_p == 32 && L.cin == 32 && L.cout == 32)
      e = hipMalloc(&L.wx, amx::conv_zx_packed_bytes());
    if (e == hipSuccess && !is_mx(cfg->precision) && L.after_up && cfg->interp == AMX_INTERP_NEAREST && L.wpk_up == nullptr && L.cout_p == L.cout &&
        amx::conv_upmerge_eligible(L.cout, L.cin - L.cout, L.cout, w_at, w_at, w_at, 1, is_split(cfg->precision))) {
      e = hipMalloc(&L.wpk_skip, (size_t)L.cout * L.cout * 28 * 2 * (is_split(cfg->precision) ? 2 : 1));
      if (e == hipSuccess) e = hipMalloc(&L.wpk_merge, amx::conv_upmerge_packed_bytes(L.cin - L.cout, L.cout, is_split(cfg->precision)));
    }
    if (e == hipSuccess && cfg->norm == AMX_NORM_BATCH_EVAL && L.norm_idx >= 0) e = hipMalloc(&L.wpk_raw, wbytes);
    if (e == hipSuccess) e = hipMalloc((void**)&L.scale, L.cout_p * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&L.shift, L.cout_p * sizeof(float));
    if (e == hipSuccess) e = hipMemset(L.scale, 0, L.cout_p * sizeof(float));      // padded channels: gain 0, shift 0 -> exact zeros
    if (e == hipSuccess) e = hipMemset(L.shift, 0, L.cout_p * sizeof(float));
    if (e == hipSuccess && cfg->norm == AMX_NORM_INSTANCE_AFFINE && L.norm_idx >= 0) {
      e = hipMalloc((void**)&L.in_gamma, L.cout_p * sizeof(float));
      if (e == hipSuccess) e = hipMalloc((void**)&L.in_beta, L.cout_p * sizeof(float));
      if (e == hipSuccess) e = hipMemset(L.in_gamma, 0, L.cout_p * sizeof(float));
      if (e == hipSuccess) e = hipMemset(L.in_beta, 0, L.cout_p * sizeof(float));
    }
    if (e != hipSuccess) {
      amx_unet_destroy(h);
      return fail(AMX_ERR_HIP, "hipMalloc: %s", hipGetErrorString(e));
    }
  }
  hipError_t e = hipMalloc((void**)&h->d_flags, amx_unet::kFlagSlots * sizeof(int));
  if (e == hipSuccess) e = hipMemset(h->d_flags, 0, amx_unet::kFlagSlots * sizeof(int));
  h->d_flag = h->d_flags;
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_flag, sizeof(int), hipHostMallocDefault);
  if (e != hipSuccess) {
    amx_unet_destroy(h);
    return fail(AMX_ERR_HIP, "hipMalloc (status flag): %s", hipGetErrorString(e));
  }
  *h->h_flag = 0;
  if (hipHostGetDevicePointer((void**)&h->h_flag_dev, h->h_flag, 0) != hipSuccess) h->h_flag_dev = nullptr;
  *out = h;
  return AMX_OK;
}

void amx_unet_destroy(amx_unet_t* h) {
  if (!h) return;
  if (h->d_flags) (void)hipFree(h->d_flags);
  if (h->h_flag) (void)hipHostFree(h->h_flag);
  for (int i = 0; i < 2; ++i)
    if (h->acc_done[i]) (void)hipEventDestroy(h->acc_done[i]);
  h->sw_lanes.release();
  h->sw_map.release();
  for (ConvLayer& L : h->convs) {
    if (L.wpk) (void)hipFree(L.wpk);
    if (L.wpk_up) (void)hipFree(L.wpk_up);
    if (L.wpk_raw) (void)hipFree(L.wpk_raw);
    if (L.mxs) (void)hipFree(L.mxs);
    if (L.wx) (void)hipFree(L.wx);
    if (L.wpk_skip) (void)hipFree(L.wpk_skip);
    if (L.wpk_merge) (void)hipFree(L.wpk_merge);
    if (L.scale) (void)hipFree(L.scale);
    if (L.in_gamma) (void)hipFree(L.in_gamma);
    if (L.in_beta) (void)hipFree(L.in_beta);
    if (L.shift) (void)hipFree(L.shift);
  }
  delete h;
}

int amx_unet_num_modules(const amx_unet_t* h) { return h ? (int)h->kinds.size() : fail(AMX_ERR_INVALID, "null handle"); }
int amx_unet_num_convs(const amx_unet_t* h) { return h ? (int)h->convs.size() : fail(AMX_ERR_INVALID, "null handle"); }

int amx_unet_conv_info(const amx_unet_t* h, int conv, int* module_idx, int* cin, int* cout, int* norm_module_idx) {
  if (!h || conv < 0 || conv >= (int)h->convs.size()) return fail(AMX_ERR_INVALID, "bad conv index %d", conv);
  const ConvLayer& L = h->convs[conv];
  if (module_idx) *module_idx = L.module_idx;
  if (cin) *cin = L.cin;
  if (cout) *cout = L.cout;
  if (norm_module_idx) *norm_module_idx = L.norm_idx;
  return AMX_OK;
}

int amx_unet_load_conv(amx_unet_t* h, int module_idx, const float* d_weight, const float* d_bias,
                       const float* d_gamma, const float* d_beta, const float* d_mean, const float* d_var,
                       void* stream) {
  if (!h || !d_weight) return fail(AMX_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  for (ConvLayer& L : h->convs) {
    if (L.module_idx != module_idx) continue;
    const bool bn = L.norm_idx >= 0 && h->cfg.norm == AMX_NORM_BATCH_EVAL;
    if (bn && (!d_mean || !d_var)) return fail(AMX_ERR_INVALID, "model.%d: BatchNorm running stats required", module_idx);
    L.raw_has_bias = bn && d_bias != nullptr;
    AMX_HIP(amx::launch_fold_norm(bn ? d_gamma : nullptr, bn ? d_beta : nullptr, bn ? d_mean : nullptr,
                                  bn ? d_var : nullptr, d_bias, h->cfg.norm_eps, L.cout, L.scale, L.shift, st));
    if (L.in_gamma) {   // InstanceNorm3d(affine=True): keep its weight / bias for the normalisation pass
      if (!d_gamma || !d_beta) return fail(AMX_ERR_INVALID, "model.%d: instance_affine needs the norm weight and bias", module_idx);
      AMX_HIP(hipMemcpyAsync(L.in_gamma, d_gamma, L.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
      AMX_HIP(hipMemcpyAsync(L.in_beta, d_beta, L.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    if (L.cin == 1 && &L == &h->convs[0]) {   // stem: 27 taps packed into one K = 32 MFMA step
      AMX_HIP(amx::launch_pack_stem(d_weight, L.scale, L.wpk, L.cout_p, stem_precision(h->cfg.precision), st, L.cout));
      if (L.wpk_raw) AMX_HIP(amx::launch_pack_stem(d_weight, nullptr, L.wpk_raw, L.cout_p, stem_precision(h->cfg.precision), st, L.cout));
    } else if (is_mx(h->cfg.precision)) {
      AMX_HIP(amx::launch_pack_weights_mx(d_weight, L.scale, L.wpk, L.mxs, L.cin, L.cin_pad, L.cout_p, L.q, st, L.cout, 0, L.c0_real, L.c0_p));
      if (L.wx) AMX_HIP(amx::launch_pack_weights_zx(d_weight, L.scale, L.wx, L.mxs, L.cout, st));      // (after: it reads the layer's max |w|)
    } else {
      if (L.wpk_raw)
        AMX_HIP(amx::launch_pack_weights(d_weight, nullptr, L.wpk_raw, L.cin, L.cin_pad, L.cout_p, L.q, h->cfg.precision, st, 0, L.cout,
                                         0, L.c0_real, L.c0_p));
      AMX_HIP(amx::launch_pack_weights(d_weight, L.scale, L.wpk, L.cin, L.cin_pad, L.cout_p, L.q,
                                       h->cfg.precision, st, 0, L.cout, 0, L.c0_real, L.c0_p));
      if (L.wpk_up) AMX_HIP(amx::launch_pack_upcat16(d_weight, L.scale, L.wpk_up, h->cfg.precision, st));
      if (L.wpk_merge) {   // skip channels [0, cout) as an ordinary 27-tap packing, upsampled channels [cout, cin) merged
        AMX_HIP(amx::launch_pack_weights(d_weight, L.scale, L.wpk_skip, L.cout, L.cout, L.cout, L.q, h->cfg.precision, st, 0, 0, L.cin));
        AMX_HIP(amx::launch_pack_upmerge(d_weight, L.scale, L.wpk_merge, L.cout, L.cin, L.cin - L.cout, L.cout, h->cfg.precision, st));
      }
    }
    L.loaded = true;
    return AMX_OK;
  }
  return fail(AMX_ERR_INVALID, "model.%d is not a convolution of this network", module_idx);
}

size_t amx_unet_workspace_bytes(const amx_unet_t* h, int n, int d, int hh, int w) { return h ? layout(h, n, d, hh, w).total : 0; }

int amx_unet_forward(amx_unet_t* h, const float* d_x, float* d_y, int n, int d, int hh, int w,
                     void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!h || !d_x || !d_y || !d_workspace) return fail(AMX_ERR_INVALID, "null argument");
  return run_forward(h, dense_args(h, d_x, d_y, n, d, hh, w, d_workspace, workspace_bytes, stream));
}

int amx_unet_module_info(const amx_unet_t* h, int module_idx, int* channels, int* level) {
  if (!h || module_idx < 0 || module_idx >= (int)h->kinds.size()) return fail(AMX_ERR_INVALID, "bad module index %d", module_idx);
  if (channels) *channels = h->mod_c[module_idx];
  if (level) *level = h->mod_level[module_idx];
  return AMX_OK;
}

int amx_unet_forward_taps(amx_unet_t* h, const float* d_x, float* d_y, int n, int d, int hh, int w,
                          void* d_workspace, size_t workspace_bytes, const int* tap_modules, int n_taps,
                          float* const* d_tap_out, int stop_module, void* stream) {
  if (!h || !d_x || !d_y || !d_workspace || n_taps < 0 || (n_taps && (!tap_modules || !d_tap_out)))
    return fail(AMX_ERR_INVALID, "null argument");
  const int nmod = (int)h->kinds.size();
  for (int t = 0; t < n_taps; ++t) {
    if (tap_modules[t] < 0 || tap_modules[t] >= nmod || !d_tap_out[t] || (t && tap_modules[t] <= tap_modules[t - 1]))
      return fail(AMX_ERR_INVALID, "tap modules must be strictly ascending ids in [0,%d) with non-null buffers", nmod);
  }
  if (stop_module >= nmod) return fail(AMX_ERR_INVALID, "stop_module %d out of range", stop_module);
  TapReq req{tap_modules, n_taps, d_tap_out, stop_module < 0 ? -1 : stop_module};
  ForwardArgs a = dense_args(h, d_x, d_y, n, d, hh, w, d_workspace, workspace_bytes, stream);
  a.taps = &req;
  return run_forward(h, a);
}

int amx_unet_forward_profiled(amx_unet_t* h, const float* d_x, float* d_y, int n, int d, int hh, int w,
                              void* d_workspace, size_t workspace_bytes, void* stream,
                              amx_launch_record* records, int max_records, int* n_records) {
  if (!h || !d_x || !d_y || !d_workspace || !records || !n_records) return fail(AMX_ERR_INVALID, "null argument");
  Profiler prof;
  prof.st = (hipStream_t)stream;
  ForwardArgs a = dense_args(h, d_x, d_y, n, d, hh, w, d_workspace, workspace_bytes, stream);
  a.prof = &prof;
  int rc = run_forward(h, a);
  if (rc == AMX_OK) {
    amx_launch_record endr;
    memset(&endr, 0, sizeof endr);
    if (prof.mark(endr)) rc = fail(AMX_ERR_HIP, "hipEventRecord failed");
  }
  if (hipStreamSynchronize(prof.st) != hipSuccess && rc == AMX_OK) rc = fail(AMX_ERR_HIP, "hipStreamSynchronize failed");
  int cnt = 0;
  if (rc == AMX_OK) {
    for (size_t k = 0; k + 1 < prof.ev.size() && cnt < max_records; ++k) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, prof.ev[k], prof.ev[k + 1]);
      prof.rec[k].ms = ms;
      records[cnt++] = prof.rec[k];
    }
  }
  for (hipEvent_t e : prof.ev) (void)hipEventDestroy(e);
  *n_records = cnt;
  return rc;
}

int amx_unet_forward_window(amx_unet_t* h, const float* d_vol, int vd, int vh, int vw, int oz, int oy,
                            int ox, int rd, int rh, int rw, const float* d_wmap, float* d_acc,
                            void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!h || !d_vol || !d_acc || !d_wmap || !d_workspace) return fail(AMX_ERR_INVALID, "null argument");
  const int corner[3] = {oz, oy, ox};
  long long off;
  if (int rc = amx::sw_window_offsets(vd, vh, vw, rd, rh, rw, 1, corner, &off)) return rc;
  const long long vvox = (long long)vd * vh * vw;
  return run_forward(h, ForwardArgs{d_vol + off, vvox * 4, (long long)vh * vw * 4, (long long)vw * 4, d_acc + off,
                                    vvox * h->cfg.output_nc, vvox, (long long)vh * vw, vw, d_wmap, 1, rd, rh, rw,
                                    d_workspace, workspace_bytes, (hipStream_t)stream});
}

// a batch of windows of one volume (acc_gate / acc_done: see ForwardArgs)
static int forward_windows(amx_unet* h, const float* d_vol, int vd, int vh, int vw, int n_windows, const int* offsets_zyx, int rd, int rh,
                           int rw, const float* d_wmap, float* d_acc, void* d_workspace, size_t workspace_bytes, void* stream,
                           hipEvent_t acc_gate, hipEvent_t acc_done) {
  if (!h || !d_vol || !d_acc || !d_wmap || !d_workspace || !offsets_zyx) return fail(AMX_ERR_INVALID, "null argument");
  if (n_windows < 1 || n_windows > 64) return fail(AMX_ERR_INVALID, "1 <= n_windows <= 64 (got %d)", n_windows);
  long long offs[64];
  if (int rc = amx::sw_window_offsets(vd, vh, vw, rd, rh, rw, n_windows, offsets_zyx, offs)) return rc;
  const long long vvox = (long long)vd * vh * vw;
  return run_forward(h, ForwardArgs{d_vol, vvox * 4, (long long)vh * vw * 4, (long long)vw * 4, d_acc, vvox * h->cfg.output_nc, vvox,
                                    (long long)vh * vw, vw, d_wmap, n_windows, rd, rh, rw, d_workspace, workspace_bytes,
                                    (hipStream_t)stream, nullptr, offs, offs, nullptr, acc_gate, acc_done});
}

int amx_unet_forward_windows(amx_unet_t* h, const float* d_vol, int vd, int vh, int vw, int n_windows,
                             const int* offsets_zyx, int rd, int rh, int rw, const float* d_wmap, float* d_acc,
                             void* d_workspace, size_t workspace_bytes, void* stream) {
  return forward_windows(h, d_vol, vd, vh, vw, n_windows, offsets_zyx, rd, rh, rw, d_wmap, d_acc, d_workspace, workspace_bytes, stream,
                         nullptr, nullptr);
}

int amx_unet_forward_windows_pipelined(amx_unet_t* h, const float* d_vol, int vd, int vh, int vw, int n_windows,
                                       const int* offsets_zyx, int rd, int rh, int rw, const float* d_wmap, float* d_acc,
                                       void* d_workspace, size_t workspace_bytes, int slot, void* stream) {
  if (!h) return fail(AMX_ERR_INVALID, "null handle");
  if (slot != 0 && slot != 1) return fail(AMX_ERR_INVALID, "slot must be 0 or 1 (got %d)", slot);
  for (int i = 0; i < 2; ++i)
    if (!h->acc_done[i]) AMX_HIP(hipEventCreateWithFlags(&h->acc_done[i], hipEventDisableTiming));
  // the other slot's event may never have been recorded yet: the wait is then a no-op
  return forward_windows(h, d_vol, vd, vh, vw, n_windows, offsets_zyx, rd, rh, rw, d_wmap, d_acc, d_workspace, workspace_bytes, stream,
                         h->acc_done[slot ^ 1], h->acc_done[slot]);
}

size_t amx_sliding_window_workspace_bytes(const amx_unet_t* h, int n_batch, int rd, int rh, int rw) {
  return h ? 2 * align_up(layout(h, n_batch, rd, rh, rw).total, 256) : 0;
}

int amx_sliding_window(amx_unet_t* h, const float* d_vol, int vd, int vh, int vw, int rd, int rh, int rw, double overlap,
                       int mode, double sigma_scale, int n_batch, int out_kind, const float* d_w, const float* d_b,
                       int classes, float* d_acc, float* d_cnt, void* d_out, void* d_workspace, size_t workspace_bytes,
                       void* stream) {
  if (!h || !d_vol || !d_acc || !d_cnt || !d_workspace) return fail(AMX_ERR_INVALID, "null argument");
  const amx_unet_cfg& c = h->cfg;
  size_t slot_bytes = 0;      // one batch's workspace: the caller's holds two, one per slot
  amx::SwNet net{"amx_sliding_window", "", c.output_nc, 64, {rd, rh, rw}, 4};
  net.check = [&](int k) {
    if (c.input_nc != 1) return fail(AMX_ERR_SHAPE, "the sliding-window call needs input_nc == 1 (got %d)", c.input_nc);
    if (c.output_nc % 16 || c.output_nc > 32)
      return fail(AMX_ERR_SHAPE, "the sliding-window call accumulates output_nc = 16 or 32 channels (got %d): use the window loop of the caller", c.output_nc);
    if (rw < 32) return fail(AMX_ERR_SHAPE, "the sliding-window call needs roi width >= 32 (got %d)", rw);
    if (int rc = check_shape(h, k, rd, rh, rw)) return rc;
    for (const ConvLayer& L : h->convs)
      if (!L.loaded) return fail(AMX_ERR_NOT_LOADED, "conv model.%d has no parameters", L.module_idx);
    slot_bytes = align_up(layout(h, k, rd, rh, rw).total, 256);
    const size_t need = amx_sliding_window_workspace_bytes(h, n_batch, rd, rh, rw);
    if (workspace_bytes < need || ((uintptr_t)d_workspace & 255))
      return fail(AMX_ERR_WORKSPACE, "workspace needs %zu bytes, 256-byte aligned (got %zu)", need, workspace_bytes);
    return pending_numerics_error(h);
  };
  net.run = [&](int nw, const int* offs, int slot, hipStream_t st) {
    if (slot < 0) return forward_windows(h, d_vol, vd, vh, vw, nw, offs, rd, rh, rw, h->sw_map.map, d_acc, d_workspace, slot_bytes, st, nullptr, nullptr);
    return amx_unet_forward_windows_pipelined(h, d_vol, vd, vh, vw, nw, offs, rd, rh, rw, h->sw_map.map, d_acc,
                                              (char*)d_workspace + slot * slot_bytes, slot_bytes, slot, st);
  };
  return amx::sw_run(net, h->sw_map, &h->sw_lanes, vd, vh, vw, overlap, mode, sigma_scale, n_batch, out_kind, d_w, d_b, classes, d_acc, d_cnt,
                     d_out, (hipStream_t)stream);
}

}  // extern "C"

