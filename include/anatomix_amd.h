/* anatomix_amd -- public C ABI of the MI355X (gfx950) anatomix UNet feature-extraction path.
 *
 * The reference (neel-dey/anatomix) is pure Python and has no FFI: its boundary for this path is
 * the nn.Module surface of anatomix.model.network.Unet.  Each entry point below names the
 * reference interface it stands in for (paths relative to the reference checkout).  The Python
 * mirror anatomix_amd.model.network.Unet binds these symbols with ctypes.
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer owned by the caller (PyTorch's allocator);
 *     the library owns only its packed-weight buffers (allocated at amx_unet_create/load);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously on it and
 *     the library never synchronises, so calls are capturable in a hipGraph;
 *   - every function returns 0 on success or a negative amx_status; amx_last_error() gives the
 *     message of the last failure on the calling thread.  Nothing aborts or throws;
 *   - a handle is not thread-safe; use one handle per module per device.
 */
#ifndef ANATOMIX_AMD_H
#define ANATOMIX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMX_VERSION 100 /* 0.1.0 */

typedef enum amx_status {
  AMX_OK = 0,
  AMX_ERR_INVALID = -1,     /* bad argument / unsupported configuration */
  AMX_ERR_SHAPE = -2,       /* spatial size not divisible by 2^num_downs, bottleneck < 2, ... */
  AMX_ERR_NOT_LOADED = -3,  /* forward before every conv received its parameters */
  AMX_ERR_WORKSPACE = -4,   /* workspace too small / misaligned */
  AMX_ERR_HIP = -5,         /* a HIP runtime call failed */
  AMX_ERR_OVERFLOW = -6     /* f16 / f16x2 storage: a value outside the f16 range (or a NaN) was produced */
} amx_status;

enum { AMX_NORM_NONE = 0, AMX_NORM_BATCH_EVAL = 1, AMX_NORM_INSTANCE = 2, AMX_NORM_INSTANCE_AFFINE = 3 };
enum { AMX_ACT_NONE = 0, AMX_ACT_RELU = 1, AMX_ACT_LRELU = 2 };
enum { AMX_POOL_MAX = 0, AMX_POOL_AVG = 1 };
enum { AMX_INTERP_NEAREST = 0, AMX_INTERP_TRILINEAR = 1 };
/* Storage precision of activations and packed weights (every MFMA accumulates in fp32).
 *   F16 / BF16     one 16-bit value per element;
 *   F16X2 / BF16X2 "strict": every element is a hi + lo pair of 16-bit values (22 / 16 mantissa bits), a voxel stores
 *                  [hi(C) | lo(C)], each product runs as three MFMAs (Wh*xh + Wh*xl + Wl*xh).  fp32-grade results --
 *                  the reference's inference callers run the network in fp32
 *                  (anatomix/registration/convex_adam_utils.py:194-219: .float().cuda(), no autocast).  BF16X2 keeps
 *                  fp32's exponent range; F16X2 is ~8x more accurate but overflows beyond 65504 like F16.
 *   F16X2_MX       strict storage (f16 hi + lo pairs) whose two CORRECTION products run on the block-scaled fp8 matrix
 *                  instruction of CDNA4 at twice the f16 rate: Wh*xh on the f16 MFMA, Wh*xl + Wl*xh from e4m3 copies the
 *                  producing kernels store beside the pair (6C bytes per voxel, row-planar: see below).  2.0 instead of 3.0
 *                  MFMA-equivalents per product; operands carry 15-16 significant bits instead of 22: the InstanceNorm
 *                  variant `anatomix-dev` stays inside the 1e-3 tolerance of the fp32 reference. */
enum { AMX_PREC_F16 = 0, AMX_PREC_BF16 = 1, AMX_PREC_F16X2 = 2, AMX_PREC_BF16X2 = 3, AMX_PREC_F16X2_MX = 4 };
/* Tensor layouts of the single-operator entries below.  F16 .. BF16X2: channels-last voxels, [n][d][h][w][c] (x2 in the strict
 * precisions: [hi(c) | lo(c)]).  F16X2_MX: ROW-PLANAR, 6 c bytes per voxel -- a row (n, z, y) of w voxels is 3 c/16 planes of w x 32
 * bytes: plane k = the f16 hi halves of channels 16k .. 16k+15 of the row's voxels, plane c/16 + k their lo halves, plane 2 c/16 + k
 * the e4m3 copies [e4m3(2^11 lo) x 16 | e4m3(hi) x 16]; so the 32 bytes per voxel that a convolution stage gathers are contiguous
 * along x.  Convolutions read hi and the copies; norm apply / pool / upsample write all three; a convolution writes hi and lo only
 * (its output is normalised before the next convolution reads it).  amx_instance_norm, which has no row length, takes a sample as
 * one row of `voxels` voxels. */

/* Constructor arguments of anatomix/model/network.py:262-279 (Unet.__init__) that shape the
 * arithmetic.  dimension is fixed at 3, pad_type at 'reflect', residual_connection at False. */
typedef struct amx_unet_cfg {
  int32_t input_nc;       /* network.py:265; 1 .. 16 (the fused sliding-window entries need 1) */
  int32_t output_nc;      /* network.py:266; any positive count (the sliding-window accumulation needs <= 32) */
  int32_t num_downs;      /* network.py:267 */
  int32_t ngf;            /* network.py:268; 8, 16, 24 (the reference default) or 32 */
  int32_t norm;           /* AMX_NORM_*   <- norm=      network.py:269,127-168 */
  float norm_eps;         /*              <- norm_eps=  network.py:278 */
  int32_t activation;     /* AMX_ACT_*    <- activation= network.py:271,171-204 */
  float act_slope;        /* 0.3 for 'lrelu' (network.py:191) */
  int32_t final_act;      /* AMX_ACT_*    <- final_act= network.py:270 */
  int32_t pooling;        /* AMX_POOL_*   <- pooling=   network.py:275,297 */
  int32_t interp;         /* AMX_INTERP_* <- interp=    network.py:276,407 */
  int32_t doubleconv;     /* network.py:273 */
  int32_t use_skip;       /* network.py:277 */
  int32_t precision;      /* AMX_PREC_*: storage type of activations / weights (fp32 accumulate); the *X2 values are the
                           * strict mode that meets the reference's fp32 results to ~1e-5 */
} amx_unet_cfg;

typedef struct amx_unet amx_unet_t;

int amx_version(void);

/* Test aid (no reference counterpart): overwrites the LDS of every compute unit with `pattern` (one 160 KB workgroup per CU, twice over),
 * so that a test can show that a kernel's results do not depend on what the previous kernel left there (tests/test_stem_fused_gpu.py). */
int amx_debug_fill_lds(unsigned pattern, void* stream);
const char* amx_last_error(void);

/* Unet.__init__ (network.py:262-465): builds the layer plan (same module indices as the
 * reference's nn.Sequential) and allocates packed-weight storage on the current device. */
int amx_unet_create(amx_unet_t** out, const amx_unet_cfg* cfg);
void amx_unet_destroy(amx_unet_t* h);

/* Layer plan queries: number of children of Unet.model, and per conv its module index
 * (the `i` of state_dict key `model.{i}.weight`), channel counts and the index of the norm
 * module that follows it (-1 if none). */
int amx_unet_num_modules(const amx_unet_t* h);
int amx_unet_num_convs(const amx_unet_t* h);
int amx_unet_conv_info(const amx_unet_t* h, int conv, int* module_idx, int* cin, int* cout, int* norm_module_idx);

/* nn.Module.load_state_dict for one Conv3d (+ the BatchNorm3d that follows it), see
 * anatomix/model/load_from_hf.py:39-49.  d_weight is fp32 [Cout][Cin][3][3][3]; d_bias (conv
 * bias), d_gamma/d_beta (norm affine), d_mean/d_var (BatchNorm running stats) are fp32 [Cout]
 * or NULL.  Eval-mode BatchNorm is folded into the packed weights here. */
int amx_unet_load_conv(amx_unet_t* h, int module_idx, const float* d_weight, const float* d_bias,
                       const float* d_gamma, const float* d_beta, const float* d_mean,
                       const float* d_var, void* stream);

/* One record per kernel launch of a profiled forward (amx_unet_forward_profiled). */
typedef struct amx_launch_record {
  char kernel[64];      /* kernel template instance, e.g. "conv3d_k3<f16,1x8x32,q1,nch1,o0>" */
  int32_t module_idx;   /* index of the conv / pool module in Unet.model */
  int32_t cin, cout;    /* logical input / output channels */
  int32_t n, d, h, w;   /* output extent of the launch */
  float ms;             /* hipEvent time from this launch to the next (includes the boundary) */
  double flops;         /* algorithmic: 2*27*cin*cout*voxels (0 for pools) */
  double bytes;         /* algorithmic: input read once + output written once + weights */
} amx_launch_record;

/* Bytes of scratch the forward needs for a batch of n volumes of d x h x w. */
size_t amx_unet_workspace_bytes(const amx_unet_t* h, int n, int d, int w_h, int w_w);

/* Unet.forward(input) standard branch (network.py:530-548), eval mode.
 * d_x: fp32 [n][input_nc][d][h][w]; d_y: fp32 [n][output_nc][d][h][w] (both NCDHW contiguous). */
int amx_unet_forward(amx_unet_t* h, const float* d_x, float* d_y, int n, int d, int hh, int w,
                     void* d_workspace, size_t workspace_bytes, void* stream);

/* Range safety of the f16 / f16x2 storage modes.  f16 overflows at 65504; folded BatchNorm gains of a real checkpoint are
 * unbounded, and an Inf that meets a ReLU or a max-pool can come out finite and wrong.  Every epilogue that stores f16
 * values therefore tests them, and when one is out of range (or NaN):
 *   - the forward that produced it has its output tensor overwritten with NaN on the device (last launch of the
 *     forward; sliding-window accumulation volumes are the caller's and are covered by the status call);
 *   - the NEXT call on this handle, or this function, returns AMX_ERR_OVERFLOW once (amx_last_error says which mode to
 *     switch to) and clears the condition.
 * synchronize != 0 waits for `stream` first, so the answer covers every forward enqueued so far.  bf16 / bf16x2 keep
 * fp32's exponent range (they overflow where the fp32 reference does) and never raise it. */
int amx_unet_numerics_status(amx_unet_t* h, int synchronize, void* stream);

/* Channels and resolution level (spatial size = input size >> level) of `feat` after Unet.model[module_idx]
 * as Unet.forward's `layers` branch sees it: for an nn.Upsample id that is AFTER torch.cat((skip, up), 1)
 * (network.py:500-502). */
int amx_unet_module_info(const amx_unet_t* h, int module_idx, int* channels, int* level);

/* Unet.forward(input, layers, encode_only) (network.py:475-529), eval mode.  tap_modules: HOST array of n_taps
 * module ids, strictly ascending (the reference collects in traversal order whatever the order of `layers`);
 * d_tap_out: HOST array of n_taps device buffers, fp32 NCDHW [n][channels][d>>level][h>>level][w>>level] per
 * amx_unet_module_info.  stop_module >= 0 reproduces encode_only: the forward ends after that module (d_y is
 * then left untouched unless the network got that far), modules after it do not run -- in particular an in-place
 * activation that would otherwise overwrite the tapped tensor.  Tap semantics follow the reference exactly:
 *   conv id followed by a norm ........ the pre-norm convolution output;
 *   norm id followed by an activation . the ACTIVATED tensor (nn.ReLU(inplace=True) aliases it, network.py:188-196);
 *   activation / pool id .............. that module's output;   upsample id: the concatenated tensor. */
int amx_unet_forward_taps(amx_unet_t* h, const float* d_x, float* d_y, int n, int d, int hh, int w,
                          void* d_workspace, size_t workspace_bytes, const int* tap_modules, int n_taps,
                          float* const* d_tap_out, int stop_module, void* stream);

/* Same forward, with a hipEvent recorded on `stream` around every launch; synchronises the
 * stream before returning and fills up to max_records records (profiling aid for bench.py's
 * roofline figures -- not used in the timed region). */
int amx_unet_forward_profiled(amx_unet_t* h, const float* d_x, float* d_y, int n, int d, int hh, int w,
                              void* d_workspace, size_t workspace_bytes, void* stream,
                              amx_launch_record* records, int max_records, int* n_records);

/* One sliding-window step of monai.inferers.sliding_window_inference as called from
 * anatomix/registration/convex_adam_utils.py:202-219: runs the forward on the roi-sized window of
 * volume d_vol (fp32 [vd][vh][vw], single channel) whose corner is (oz,oy,ox) and accumulates
 *   d_acc[c][oz+z][oy+y][ox+x] += d_wmap[z][y][x] * feature[c][z][y][x]
 * (d_acc fp32 [output_nc][vd][vh][vw]).  Windows that overlap must be issued on one stream. */
int amx_unet_forward_window(amx_unet_t* h, const float* d_vol, int vd, int vh, int vw, int oz, int oy,
                            int ox, int rd, int rh, int rw, const float* d_wmap, float* d_acc,
                            void* d_workspace, size_t workspace_bytes, void* stream);

/* n_windows sliding-window steps in one call (the reference hands sw_batch_size windows to the predictor at a
 * time, convex_adam_utils.py:205; any batching gives the same result because every norm mode is per sample or
 * uses running statistics).  offsets_zyx: HOST array [n_windows][3] of window corners.  The stem and the output
 * convolution run once per window in the given order (so overlapping accumulations are ordered on the stream);
 * all layers between them run on the whole batch.  Workspace: amx_unet_workspace_bytes(h, n_windows, rd, rh, rw). */
int amx_unet_forward_windows(amx_unet_t* h, const float* d_vol, int vd, int vh, int vw, int n_windows,
                             const int* offsets_zyx, int rd, int rh, int rw, const float* d_wmap, float* d_acc,
                             void* d_workspace, size_t workspace_bytes, void* stream);

/* Two window batches in flight.  Same as amx_unet_forward_windows, for a caller that alternates TWO streams (and two
 * workspaces) over consecutive window batches: slot = 0 / 1 alternately.  Everything up to the output conv of batch k+1 overlaps
 * batch k; the accumulating launches of a batch first wait for the other slot's accumulations, so overlapping windows are still
 * added in window order and the result is bit-identical to the single-stream sequence.  The caller joins both streams before
 * reading d_acc.  (MONAI's sliding_window_inference runs its sw_batch groups strictly one after the other,
 * convex_adam_utils.py:205-219 is the call.) */
int amx_unet_forward_windows_pipelined(amx_unet_t* h, const float* d_vol, int vd, int vh, int vw, int n_windows,
                                       const int* offsets_zyx, int rd, int rh, int rw, const float* d_wmap, float* d_acc,
                                       void* d_workspace, size_t workspace_bytes, int slot, void* stream);

/* Final step of sliding_window_inference: d_acc[c][v] /= d_cnt[v] in place. */
int amx_sw_normalize(float* d_acc, const float* d_cnt, int channels, long long voxels, void* stream);

/* d_cnt[oz+z][oy+y][ox+x] += d_wmap[z][y][x] for one window (the count map of
 * sliding_window_inference). */
int amx_sw_count(float* d_cnt, int vd, int vh, int vw, int oz, int oy, int ox, int rd, int rh, int rw,
                 const float* d_wmap, void* stream);

/* ---- whole-volume sliding-window inference behind one call ------------------------------------------------------------
 * monai.inferers.sliding_window_inference as the reference calls it: for features at
 * anatomix/registration/convex_adam_utils.py:202-219, for the logits of a finetuned head at
 * anatomix/segmentation/train_segmentation.py:194-199.  MONAI's schedule is restated in SURVEY.md Appendix D. */
typedef enum amx_sw_map { AMX_SW_MAP_CONSTANT = 0, AMX_SW_MAP_GAUSSIAN = 1 } amx_sw_map;
typedef enum amx_sw_out {
  AMX_SW_FEATURES = 0, /* d_acc /= d_cnt in place (amx_sw_normalize's arithmetic, bit for bit); d_out is not used */
  AMX_SW_LOGITS = 1,   /* d_out fp32 [classes][V] = b + W (d_acc / d_cnt); d_acc is left as it is */
  AMX_SW_LABELS = 2    /* d_out uint8 [V] = arg-max of those logits, the lowest index on ties; they are never written */
} amx_sw_out;

/* The window corners of sliding_window_inference(..., roi_size, overlap) (convex_adam_utils.py:202-219) in MONAI's order,
 * first axis outermost.  Host only.  Per axis: scan interval int(roi * (1 - overlap)), floored at 1, roi itself when the
 * axis equals the roi; windows 0 .. d with d the first one that reaches the end, the last start being size - roi.
 * Returns the number of windows (>= 1) and writes the first min(count, capacity) corners to offsets_zyx [capacity][3]
 * (may be NULL with capacity 0).  A volume smaller than the roi on any axis is AMX_ERR_SHAPE: padding is the caller's.
 * overlap outside [0, 1) is AMX_ERR_INVALID. */
int amx_sw_plan(int vd, int vh, int vw, int rd, int rh, int rw, double overlap, int* offsets_zyx, int capacity);

/* The window weights of sliding_window_inference(mode=..., sigma_scale=...) (convex_adam_utils.py:202-219): d_wmap fp32
 * [rd][rh][rw] = 1 (AMX_SW_MAP_CONSTANT) or the separable Gaussian exp(-x^2 / (2 sigma^2)), sigma = roi * sigma_scale per
 * axis, clamped below at max(min(map), 1e-3).  May differ from a torch-built map in the last bits of expf: measured at 32^3 / 0.125
 * and 64^3 / 0.25, identical to the map torch builds on the device and within 4.3e-7 relative of the one it builds on the host. */
int amx_sw_importance_map(float* d_wmap, int rd, int rh, int rw, int mode, double sigma_scale, void* stream);

/* The count map of ALL windows of amx_sw_plan(vd, .., overlap) in one launch (the `count_map` of sliding_window_inference,
 * convex_adam_utils.py:202-219): d_cnt[v] = sum of d_wmap over the windows that cover v, added in window order from zero.
 * Every voxel of d_cnt is written; the result is bit-identical to amx_sw_count per window on a zeroed map. */
int amx_sw_count_all(float* d_cnt, int vd, int vh, int vw, int rd, int rh, int rw, double overlap, const float* d_wmap,
                     void* stream);

/* The last pass of sliding_window_inference over (d_acc fp32 [feat][voxels], d_cnt fp32 [voxels]), kind an amx_sw_out:
 * the `output_image / count_map` of convex_adam_utils.py:202-219, followed for LOGITS / LABELS by the 1x1x1 head and the
 * arg-max of train_segmentation.py:194-199 / :84-86 (a per-voxel affine head commutes with the window average).
 * d_w fp32 [classes][feat], d_b fp32 [classes] or NULL; both unused for FEATURES.  Envelope (amx_seg_argmax's):
 * 2 <= classes <= 32, 1 <= feat <= 64, AMX_ERR_INVALID outside it before anything is launched.  Any voxels count and
 * alignment. */
int amx_sw_finish(int kind, float* d_acc, const float* d_cnt, int feat, long long voxels, const float* d_w, const float* d_b,
                  int classes, void* d_out, void* stream);

/* Bytes of workspace amx_sliding_window needs: two window batches of n_batch roi-sized windows in flight (the sw_batch_size
 * windows MONAI hands to the predictor at a time, convex_adam_utils.py:202-219, twice). */
size_t amx_sliding_window_workspace_bytes(const amx_unet_t* h, int n_batch, int rd, int rh, int rw);

/* sliding_window_inference(volume, roi, n_batch, model, overlap, mode, sigma_scale) in one call
 * (convex_adam_utils.py:202-219; with a head, the validation inference of train_segmentation.py:194-199).
 * d_vol fp32 [vd][vh][vw] single channel, at least the roi on every axis (padding is the caller's).  The call zeroes
 * d_acc fp32 [output_nc][vd*vh*vw], builds the window weights (cached on the handle per roi, mode and sigma_scale; the
 * first call with a new key allocates them), writes d_cnt fp32
 * [vd*vh*vw] with amx_sw_count_all, runs the windows of amx_sw_plan in batches of n_batch (1 .. 64) through
 * amx_unet_forward_windows and ends with amx_sw_finish(out_kind, ...): features in d_acc, or logits / labels in d_out
 * (d_w, d_b, classes: the head, NULL / 0 for features).
 * With 4 or more batches two of them are kept in flight: the even ones on `stream`,
 * the odd ones on a non-blocking stream of the handle, created at the first such call, which forks from and joins
 * `stream` (amx_unet_forward_windows_pipelined's ordering: only the accumulating launches of consecutive batches are
 * ordered, the sums are those of the single-stream sequence bit for bit).  For the caller the whole call is ordered on
 * `stream`.  No host synchronisation.  While `stream` is capturing the call is refused (AMX_ERR_INVALID): its pieces
 * (amx_sw_count_all, amx_unet_forward_windows, amx_sw_finish) replay correctly from a graph, the whole call did not yet.
 * Envelope: input_nc == 1, output_nc a multiple of 16 and <= 32, rw >= 32, the roi a shape the forward takes:
 * AMX_ERR_SHAPE otherwise; too small a workspace is AMX_ERR_WORKSPACE; the head as for amx_sw_finish.  Every check
 * comes before the first launch: a refused call leaves all buffers untouched.
 * f16 / f16x2 storage: the range check stays amx_unet_numerics_status's -- call it with synchronize != 0 after this call
 * before trusting d_acc / d_out. */
int amx_sliding_window(amx_unet_t* h, const float* d_vol, int vd, int vh, int vw, int rd, int rh, int rw, double overlap,
                       int mode, double sigma_scale, int n_batch, int out_kind, const float* d_w, const float* d_b,
                       int classes, float* d_acc, float* d_cnt, void* d_out, void* d_workspace, size_t workspace_bytes,
                       void* stream);

/* Single-layer entry (per-kernel parity / roofline tests): y = act(conv3x3x3_reflect(cat(x0,
 * up2_nearest(x1))) * scale + shift).  x0: 16-bit NDHWC [n][d][h][w][c0]; x1: 16-bit NDHWC
 * [n][d/2][h/2][w/2][c1] or NULL (c1 = 0); d_weight fp32 [cout][c0+c1][27]; d_scale/d_shift fp32
 * [cout] or NULL; output 16-bit NDHWC (d_out16) or fp32 NCDHW (d_out32), exactly one non-NULL.
 * d_wpk is scratch for the packed weights: amx_conv3d_packed_bytes(c0+c1, cout) bytes. */
size_t amx_conv3d_packed_bytes(int cin, int cout);
int amx_conv3d_k3_reflect(const void* d_x0, int c0, const void* d_x1, int c1, const float* d_weight,
                          const float* d_scale, const float* d_shift, int cout, int n, int d, int hh,
                          int w, int act, float slope, int precision, void* d_wpk, void* d_out16,
                          float* d_out32, void* stream);

/* Test aid (no reference counterpart): amx_conv3d_k3_reflect with the launch-side options that only amx_unet_forward sets otherwise,
 * so that single-layer tests reach them and learn which kernel ran.  Each may be NULL: d_pool16, the fused 2x2x2 max-pool output
 * [n][d/2][hh/2][w/2][cout] (16-bit output, a z-march layer with even extents: AMX_ERR_SHAPE otherwise); d_wmap, fp32 [d][hh][w], the
 * fp32 planar epilogue then ACCUMULATES out32 += wmap * value into the caller's d_out32; d_oflow, a device int set to 1 when a value
 * about to be stored in f16 lies outside the f16 range (or is NaN); kernel_name, 64 bytes on the host, the launch's name as in
 * amx_launch_record::kernel. */
int amx_conv3d_k3_reflect_probe(const void* d_x0, int c0, const void* d_x1, int c1, const float* d_weight, const float* d_scale,
                                const float* d_shift, int cout, int n, int d, int hh, int w, int act, float slope, int precision,
                                void* d_wpk, void* d_out16, float* d_out32, void* d_pool16, const float* d_wmap, int* d_oflow,
                                char* kernel_name, void* stream);

/* The same call with caller-owned scratch for the layers that split K across workgroups (deep levels with few voxels:
 * conv3d_k3_ks writes fp32 partial tensors per K slice, a second kernel sums them in slice order -- deterministic).
 * amx_conv3d_scratch_bytes returns 0 when the shape does not split; d_scratch may then be NULL. */
size_t amx_conv3d_scratch_bytes(int c0, int c1, int cout, int n, int d, int hh, int w, int precision);
int amx_conv3d_k3_reflect_ws(const void* d_x0, int c0, const void* d_x1, int c1, const float* d_weight,
                             const float* d_scale, const float* d_shift, int cout, int n, int d, int hh,
                             int w, int act, float slope, int precision, void* d_wpk, void* d_out16,
                             float* d_out32, void* d_scratch, size_t scratch_bytes, void* stream);

/* The same convolution with a described weight tensor, so that callers need no host-side reshuffling:
 *   weight_mode 0: d_weight fp32 [cout_real][cin_real][27]; input channels cin_real .. c0+c1-1 and output channels
 *                  cout_real .. cout-1 are zero padding (the stem: one real input channel in a 16-channel tensor);
 *   weight_mode 1: DATA-GRADIENT weights taken from the forward tensor d_weight fp32 [cin_real][cout_real][27]
 *                  (= the forward conv's [Cout][Cin][27]): taps flipped, channels transposed -- run on the zero-framed
 *                  output gradient and followed by amx_pad_fold it is the adjoint of the forward conv. */
int amx_conv3d_k3_reflect_ex(const void* d_x0, int c0, const void* d_x1, int c1, const float* d_weight, int weight_mode,
                             int cin_real, int cout_real, const float* d_scale, const float* d_shift, int cout, int n,
                             int d, int hh, int w, int act, float slope, int precision, void* d_wpk, void* d_out16,
                             float* d_out32, void* stream);

/* Packing of MANY layers in one launch (the training step: every conv's weights change with every optimizer step, and packing each
 * inside its conv call put 40 small launches on the step's critical path).  Request i packs d_weight (described as for
 * amx_conv3d_k3_reflect_ex: weight_mode 0 / 1, cin_real of cin_pad stored input channels, cout_real of cout) into d_wpk
 * (amx_conv3d_packed_bytes(cin_pad, cout) bytes) for a layer of spatial WIDTH w (the tile shape -- hence the packing -- depends on
 * it).  The conv is then called with weight_mode | AMX_WEIGHTS_PREPACKED and that d_wpk (d_weight may be NULL).  Plain 16-bit
 * precisions; not for the 16 + up32 -> 16 merged-tap layer. */
#define AMX_WEIGHTS_PREPACKED 16
typedef struct amx_pack_req {
  const float* d_weight;
  void* d_wpk;
  int weight_mode, cin_real, cin_pad, cout_real, cout, w;
} amx_pack_req;
int amx_conv3d_pack_batch(const amx_pack_req* reqs, int count, int precision, void* stream);

/* Data gradient of the reflect-padded conv WITHOUT the padded-domain detour (amx_train.hip): d_dy_framed is the zero-framed output
 * gradient [n][d+4][hh+4][w+4][c_dy] (the buffer amx_bn_act_backward writes); amx_conv3d_dgrad_interior runs the forward kernel on its
 * interior with the halo read from the frame (the zero-padded correlation with the flipped, transposed FORWARD weights d_weight
 * fp32 [cin_real = forward Cout][cout_real = forward Cin][27]; weight_flags 0 or AMX_WEIGHTS_PREPACKED with a weight_mode-1 packing)
 * into the dense 16-bit d_out16 [n][d][hh][w][cout]; amx_conv3d_dgrad_fold_shell then adds the folded shell terms of the reflect
 * adjoint to the voxels with a coordinate 1 or size - 2.  Together = amx_conv3d_k3_reflect_ex(weight_mode 1) on the framed domain
 * followed by amx_pad_fold.  Shapes: what the z-march kernels take (16 / 32 channels in, 16 / 32 out, not 32 -> 16, w >= 32, d, hh >= 8):
 * amx_conv3d_dgrad_interior_supported returns 1. */
int amx_conv3d_dgrad_interior_supported(int c_dy, int cout, int d, int hh, int w, int precision);
int amx_conv3d_dgrad_interior(const void* d_dy_framed, int c_dy, const float* d_weight, int weight_flags, int cin_real, int cout_real, int cout,
                              int n, int d, int hh, int w, int precision, void* d_wpk, void* d_out16, void* stream);
size_t amx_conv3d_dgrad_shell_scratch_bytes(void);     /* d_scratch of amx_conv3d_dgrad_fold_shell: the shell sources' MFMA fragment table */
int amx_conv3d_dgrad_fold_shell(const void* d_dy_framed, int c_dy, const float* d_weight, int co_real, int ci_real, void* d_dx, int c_dx, int n,
                                int d, int hh, int w, int precision, void* d_scratch, void* stream);

/* nn.MaxPool3d(2) / nn.AvgPool3d(2) on a 16-bit NDHWC tensor (network.py:297,368). */
int amx_pool2(const void* d_in, void* d_out, int n, int d_out_, int h_out, int w_out, int c, int avg,
              int precision, void* stream);

/* nn.InstanceNorm3d(c, eps, affine = d_gamma != NULL) followed by the activation, IN PLACE on a 16-bit NDHWC
 * tensor [n][voxels][c] (network.py:157-163: 'instance' / 'instance_affine'; biased variance over the voxels of
 * each (n, c) plane).  d_scratch: amx_instance_norm_scratch_bytes(n, c) bytes of fp32 partial sums. */
size_t amx_instance_norm_scratch_bytes(int n, int c);
int amx_instance_norm(void* d_x, const float* d_gamma, const float* d_beta, float eps, int n, long long voxels,
                      int c, int act, float slope, void* d_scratch, int precision, void* stream);

/* nn.Upsample(scale_factor=2, mode='trilinear') (align_corners=False; network.py:407): 16-bit NDHWC
 * [n][din][hin][win][c] -> [n][2 din][2 hin][2 win][c]. */
int amx_upsample2_trilinear(const void* d_in, void* d_out, int n, int din, int hin, int win, int c,
                            int precision, void* stream);

/* Test aids (no reference counterpart): the fused launches of the AMX_PREC_F16X2_MX schedule, which only amx_unet_forward makes
 * otherwise, one launch each, so that single-launch tests reach them (tests/test_mx_fused_gpu.py).  Row-planar tensors throughout
 * (uint8 [n][d][hh][3 c/16][w][32]); d_oflow, where given, is a device int set to 1 when a value about to be stored in f16 lies outside
 * the f16 range (or is NaN), may be NULL.
 *
 * amx_conv3d_zx_probe: one 32 -> 32 layer of the normalise-on-load z-march kernel.  d_x: its input, whose InstanceNorm + activation is
 * pending when d_in_ab, fp32 [n][32][2] (a, b), is given: the kernel reads act_in(a x + b) (in_act, in_slope).  d_weight fp32
 * [32][32][27], d_scale / d_bias fp32 [32] or NULL.  Exactly one output: d_out16, row-planar, the RAW convolution (pair only: the copy
 * section is not written; act must be AMX_ACT_NONE), with the InstanceNorm partial sums of (value - bias) and its square in d_stats,
 * fp32 [n][amx_conv3d_zx_probe_stats_slots(hh, w)][32][2], when that is given; or d_out32, fp32 NCDHW, which takes no statistics and
 * no activation (AMX_ERR_INVALID).  d even and >= 4, and w % 32 == 0 with hh even or w % 16 == 0 with hh % 4 == 0: AMX_ERR_SHAPE
 * otherwise, before anything is launched.  d_ws: amx_conv3d_zx_probe_workspace_bytes() bytes, 256-byte aligned, for the packings.
 * kernel_name: 64 bytes on the host, the launch's name as in amx_launch_record::kernel, or NULL. */
size_t amx_conv3d_zx_probe_workspace_bytes(void);
int amx_conv3d_zx_probe_stats_slots(int hh, int w);
int amx_conv3d_zx_probe(const void* d_x, const float* d_weight, const float* d_scale, const float* d_bias, const float* d_in_ab, int in_act,
                        float in_slope, int n, int d, int hh, int w, int act, void* d_ws, size_t ws_bytes, void* d_out16, float* d_out32,
                        float* d_stats, int* d_oflow, char* kernel_name, void* stream);

/* amx_instance_norm with every argument of its launcher: w, the row length of the row-planar layout (f16x2mx; voxels % w == 0);
 * fused_slots > 0: the statistics pass is skipped, the head of d_scratch holds partial sums [n][fused_slots][c][2] of (x - K) and its
 * square, K = d_kshift[c] (NULL: 0) -- a conv epilogue's, or the caller's; more than 512 slots are folded by a pre-reduction first;
 * apply = 0: the tensor stays as it is (d_x may then be NULL when fused_slots > 0) and the pairs (a, b) with y = a x + b go to d_ab_out,
 * fp32 [n][c][2] (NULL: they stay in the scratch); skip_lo (f16x2mx): the apply pass writes hi and the copies, not the lo planes.
 * d_scratch: amx_instance_norm_probe_scratch_bytes(n, c, fused_slots) bytes. */
size_t amx_instance_norm_probe_scratch_bytes(int n, int c, int slots);
int amx_instance_norm_probe(void* d_x, const float* d_gamma, const float* d_beta, float eps, int n, long long voxels, int c, int w, int act,
                            float slope, void* d_scratch, size_t scratch_bytes, int precision, int fused_slots, const float* d_kshift,
                            int skip_lo, int apply, float* d_ab_out, int* d_oflow, void* stream);

/* y = act(a x + b) in place on d_x [n][d][hh][w][c] with the caller's pairs d_ab fp32 [n][c][2], and its 2x2x2 average (avg) or
 * maximum pooled copy into d_pooled [n][d/2][hh/2][w/2][c], one launch.  f16x2mx only, even extents, c % 16 == 0 and w * c / 8 a
 * multiple of 64: AMX_ERR_SHAPE otherwise.  skip_lo / pool_skip_lo: the lo planes of the tensor / of the pooled copy are not written. */
int amx_instance_norm_apply_pool_probe(void* d_x, const float* d_ab, void* d_pooled, int n, int d, int hh, int w, int c, int act, float slope,
                                       int avg, int skip_lo, int pool_skip_lo, int precision, int* d_oflow, void* stream);

/* amx_upsample2_trilinear of a tensor whose InstanceNorm + activation is pending: d_ab fp32 [n][c][2] (NULL: none), the eight inputs of
 * a cell become act(a x + b) on the way in.  skip_lo (f16x2mx): the lo planes of the output are not written. */
int amx_upsample2_trilinear_pending(const void* d_in, void* d_out, int n, int din, int hin, int win, int c, int precision, int skip_lo,
                                    const float* d_ab, int act, float slope, int* d_oflow, void* stream);

/* Adjoint of torch.cat((skip, nn.Upsample(2, 'nearest')(low)), 1) (network.py:500-502, 545) applied to the data gradient of the
 * concat conv: d_dcat 16-bit [n][2 dlow][2 hlow][2 wlow][c0 + c1] -> d_dskip [n][2 dlow][2 hlow][2 wlow][c0] (first c0
 * channels; added to the existing content when accumulate_skip) and d_dlow [n][dlow][hlow][wlow][c1] (sum of the 8 children of
 * every low-resolution voxel).  One pass over d_dcat.  c0 == 0 (d_dskip may be NULL): no skip part, c0 and c1 multiples of 8. */
int amx_upcat_split_backward(const void* d_dcat, void* d_dskip, void* d_dlow, int n, int dlow, int hlow, int wlow, int c0, int c1,
                             int accumulate_skip, int precision, void* stream);
/* The same with the reflect-padding adjoint (amx_pad_fold) applied while reading: d_g_framed is the data-gradient conv's raw result
 * on the padded domain, [n][2 dlow + 4][2 hlow + 4][2 wlow + 4][c0 + c1]; the folded full-resolution gradient is never written and
 * the children are summed in fp32 before the one rounding.  c0 == 0 (d_dskip may be NULL): the tensor has no skip part. */
int amx_upcat_split_backward_framed(const void* d_g_framed, void* d_dskip, void* d_dlow, int n, int dlow, int hlow, int wlow, int c0,
                                    int c1, int accumulate_skip, int precision, void* stream);

/* Layout conversions between the library's 16-bit channels-last activations and torch's fp32 NCDHW tensors, for the
 * feature taps of the differentiable forward (network.py:475-529 returns the taps as fp32 NCDHW tensors) and their
 * gradients coming back: export  d_src 16-bit [n][d][h][w][c] -> d_out fp32 [n][c][d][h][w];
 * import  d_src fp32 [n][c][d][h][w] -> d_dst 16-bit through byte strides (voxel pitch dst_sx >= 2 c; lets the interior of
 * a zero-framed gradient buffer be the destination), adding to the destination when accumulate != 0.  c % 8 == 0. */
/* The network input for the training path: d_src fp32 [n][cin][d][hh][w] (1 <= cin <= 16) -> d_dst 16-bit channels-last
 * [n][d][hh][w][16], the real channels first and the rest zero -- one pass (the differentiable forward pads the input to one
 * 16-channel chunk so that its first conv is an ordinary 16 -> ngf layer, network.py:310-333 with input_nc = 1 or 2). */
int amx_import_input(const float* d_src, void* d_dst, int n, int cin, int d, int hh, int w, int precision, void* stream);
int amx_export_ncdhw(const void* d_src, int c, int n, int d, int hh, int w, float* d_out, int precision, void* stream);
int amx_import_ncdhw(const float* d_src, void* d_dst, int n, int c, int d, int hh, int w, long long dst_sn, long long dst_sz,
                     long long dst_sy, long long dst_sx, int accumulate, int precision, void* stream);

/* Adjoint of amx_upsample2_trilinear (autograd of nn.Upsample(2, 'trilinear'), network.py:407, in the training path):
 * d_gout 16-bit [n][2 din][2 hin][2 win][c] -> d_gin [n][din][hin][win][c]. */
int amx_upsample2_trilinear_backward(const void* d_gout, void* d_gin, int n, int din, int hin, int win, int c, int precision,
                                     void* stream);

/* The same layer as amx_conv3d_k3_reflect with c1 > 0, computed the way amx_unet_forward runs the wider nearest-upsample
 * concat layers (network.py:403-435: nn.Upsample(2,'nearest') -> torch.cat((skip, up), 1) -> nn.Conv3d(3, reflect) -> norm ->
 * act): (1) the ordinary 27-tap convolution over the skip channels writes raw partial sums into d_partial; (2) the merged-tap
 * convolution over the upsampled channels at LOW resolution -- the 27 taps over a nearest-upsampled tensor collapse to 2x2x2
 * parity-dependent taps, 3.4x fewer multiply-accumulates -- adds them, the bias and the activation.  Needs c0 == cout,
 * c1 a multiple of 32, cout >= 32 (>= 16 in the strict precisions), w >= 16, even dims; AMX_ERR_INVALID otherwise.  d_wpk:
 * amx_conv3d_upcat_merged_packed_bytes(c0, c1, cout) bytes of scratch for both packings; d_partial: n*d*h*w*cout*2 bytes. */
size_t amx_conv3d_upcat_merged_packed_bytes(int c0, int c1, int cout);
int amx_conv3d_upcat_merged(const void* d_x0, int c0, const void* d_x1, int c1, const float* d_weight, const float* d_scale,
                            const float* d_shift, int cout, int n, int d, int hh, int w, int act, float slope, int precision,
                            void* d_wpk, void* d_partial, void* d_out16, void* stream);

/* ---- Training-path operators (the UNet inside the contrastive step, pretraining/models/supcl_model.py:603-661, runs in
 * train mode and is differentiated).  All activations / gradients: dense 16-bit channels-last [n][d][h][w][c];
 * parameter gradients and statistics fp32.  d_scratch: amx_train_scratch_bytes(c) bytes. */
size_t amx_train_scratch_bytes(int c);

/* nn.BatchNorm3d in TRAIN mode + activation (network.py:148-152,171-196): y = act(gamma (x - mean) rstd + beta) with the
 * biased batch variance over n * voxels rows; saves mean / rstd (each [c], may be NULL), updates the running statistics
 * (running_var with the unbiased variance; pointers may be NULL).  d_y may equal d_x. */
int amx_bn_train_forward(const void* d_x, void* d_y, const float* d_gamma, const float* d_beta, float eps, int n,
                         long long voxels, int c, int act, float slope, void* d_scratch, float* d_save_mean,
                         float* d_save_rstd, float* d_running_mean, float* d_running_var, float momentum, int precision,
                         void* stream);

/* Adjoint of the above (and of a bare activation when d_mean == NULL): dz = dy * act'(y); dbeta = sum dz;
 * dgamma = sum dz * xhat; dx = gamma rstd (dz - dbeta / M - xhat dgamma / M), written into the INTERIOR of the zero-framed
 * buffer d_dx_framed [n][d+4][h+4][w+4][c] (the caller zeroes the frame once), the input of the data-gradient conv. */
int amx_bn_act_backward(const void* d_dy, const void* d_y, const void* d_x, const float* d_mean, const float* d_rstd,
                        const float* d_gamma, float* d_dgamma, float* d_dbeta, void* d_dx_framed, int n, int d, int hh, int w,
                        int c, int act, float slope, void* d_scratch, int precision, void* stream);
/* The same adjoint of norm + activation WITHOUT reading the activated output: act' only needs the sign of its argument, and that
 * argument is recomputed from the saved pre-norm tensor, z = a x + b with a = rstd gamma, b = beta - mean rstd gamma (the
 * coefficients amx_bn_train_forward applied; d_gamma / d_beta NULL = 1 / 0).  Each of the two passes reads two tensors instead of
 * three.  For relu / lrelu the result equals amx_bn_act_backward's wherever the stored y kept the sign of z (always in bf16; in f16
 * except for |z| below its smallest subnormal). */
int amx_bn_act_backward_recompute(const void* d_dy, const void* d_x, const float* d_mean, const float* d_rstd, const float* d_gamma,
                                  const float* d_beta, float* d_dgamma, float* d_dbeta, void* d_dx_framed, int n, int d, int hh, int w,
                                  int c, int act, float slope, void* d_scratch, int precision, void* stream);

/* Adjoint of the reflect padding of nn.Conv3d(padding='same', padding_mode='reflect') (network.py:310-318).  The data
 * gradient of the conv is amx_conv3d_k3_reflect run on the framed (d+4)(h+4)(w+4) output gradient with the weights
 * flipped along the three taps and transposed (cin <-> cout); this folds the result [n][d+4][h+4][w+4][c] back onto
 * [n][d][h][w][c]: voxel i collects padded positions i, -1 (if i == 1) and L (if i == L-2) per axis. */
int amx_pad_fold(const void* d_g_framed, void* d_din, int n, int d, int hh, int w, int c, int accumulate, int precision,
                 void* stream);

/* Adjoint of nn.MaxPool3d(2) (network.py:297,368): d_dp [n][dout][hout][wout][c] is routed to the FIRST maximum of each
 * 2x2x2 window of d_in [n][2 dout][2 hout][2 wout][c] (z, y, x order: torch's tie rule). */
int amx_pool2_max_backward(const void* d_dp, const void* d_in, void* d_din, int n, int dout, int hout, int wout, int c,
                           int accumulate, int precision, void* stream);

/* Weight gradient of nn.Conv3d(k3, reflect): d_dw fp32 [cout][cin_real][3][3][3] (+)= sum over voxels of dy (x) input.
 * d_dy: 16-bit [n][d][h][w][cout] through BYTE strides (so the interior of a framed buffer can be passed);
 * input = cat(d_x0 [c0 ch, full resolution], nearest-upsampled d_x1 [c1 ch, half resolution]) as in the forward;
 * cin_real <= c0 + c1 trims zero-padded input channels (the stem: 1 real channel padded to 16). */
size_t amx_conv3d_wgrad_scratch_bytes(int n, int d, int hh, int w, int cout, int cin_pad);
int amx_conv3d_wgrad(const void* d_dy, long long dy_sn, long long dy_sz, long long dy_sy, long long dy_sx, const void* d_x0,
                     int c0, const void* d_x1, int c1, int cin_real, int cout, int n, int d, int hh, int w, float* d_dw,
                     int accumulate, void* d_scratch, size_t scratch_bytes, int precision, void* stream);

/* Fused attention core of the 3D ViT variant `anatomix-dev-vit` (PrimusV2-S: anatomix/model/vit3d/architectures.py:231-260,
 * registry entry load_from_hf.py:25-35; the blocks themselves live in the third-party dynamic-network-architectures / timm
 * packages, see oracle/vit_ref.py).  Replaces, inside every EVA block, the sequence
 *     q, k = q_norm(q), k_norm(k)                  per-head nn.LayerNorm(head_dim), the wrapper's qk_norm (architectures.py:108-115)
 *     q, k = rope(q), rope(k)                      on the tokens after the n_prefix register tokens (x*cos + rot(x)*sin)
 *     out  = softmax(q k^T / sqrt(head_dim)) v     torch F.scaled_dot_product_attention
 * d_q / d_k / d_v / d_out: fp32 [b][n][heads*head_dim] (the layout the q / k / v projections produce and the output
 * projection consumes).  d_*n_w / d_*n_b: fp32 [head_dim] or NULL (no QK norm).  d_rope: fp32 [n - n_prefix][2*head_dim] =
 * per token [sin | cos], or NULL.  head_dim even, <= 80.  f16 MFMA operands, fp32 LayerNorm / rotation / softmax / accumulate. */
size_t amx_attention_scratch_bytes(int b, int heads, int n, int head_dim);
int amx_attention_qknorm_rope(const float* d_q, const float* d_k, const float* d_v, const float* d_qn_w, const float* d_qn_b,
                              const float* d_kn_w, const float* d_kn_b, float norm_eps, const float* d_rope, int n_prefix, int b,
                              int n, int heads, int head_dim, float* d_out, void* d_scratch, size_t scratch_bytes, void* stream);

/* softmax(q k^T / sqrt(head_dim)) v alone, on the f16 operands a previous amx_attention_qknorm_rope call with the SAME
 * (b, n, heads, head_dim) left in d_scratch: the flash kernel without its preparation pass (what one EVA block of amx_vit_forward
 * launches after its q | k and v projections; bench.py times it as the ViT's dominant kernel). */
int amx_attention_prepared(const void* d_scratch, size_t scratch_bytes, int b, int n, int heads, int head_dim, float* d_out, void* stream);

/* ---- The attention core under autograd ---------------------------------------------------------------------------------------
 * Training the ViT (the reference trains it: pretraining/models/pretraining_networks.py:107-145, options/primus_options.py) needs
 * the gradient of the sequence above.  These entries replace what torch autograd records and replays for
 * q_norm / k_norm -> rope -> F.scaled_dot_product_attention: the forward that also saves the log-sum-exp, and one backward call.
 *
 * amx_attention_train_scratch_bytes: bytes of d_scratch for amx_attention_backward (0 outside the envelope: head_dim even and <= 80,
 * b, n, heads >= 1); the forward entry below needs only amx_attention_scratch_bytes of it. */
size_t amx_attention_train_scratch_bytes(int b, int heads, int n, int head_dim);
/* amx_attention_qknorm_rope (same arguments, bit-identical d_out) that also stores d_lse: fp32 [b][heads][n], the log-sum-exp of every
 * score row in the exp2 domain (scores already multiplied by log2(e) / sqrt(head_dim)) -- what autograd's SDPA node saves instead of
 * the probabilities. */
int amx_attention_qknorm_rope_train(const float* d_q, const float* d_k, const float* d_v, const float* d_qn_w, const float* d_qn_b,
                                    const float* d_kn_w, const float* d_kn_b, float norm_eps, const float* d_rope, int n_prefix, int b,
                                    int n, int heads, int head_dim, float* d_out, float* d_lse, void* d_scratch, size_t scratch_bytes,
                                    void* stream);
/* Backward of the call above (replaces the autograd nodes of F.scaled_dot_product_attention, the rotation and the two per-head
 * nn.LayerNorm): from the saved fp32 d_q / d_k / d_v, d_out, d_lse and the incoming gradient d_dout (fp32, contiguous, the layout of
 * d_out) it writes d_dq / d_dk / d_dv (the layout of d_q) and the gradients of the norm parameters d_dqn_w / d_dqn_b / d_dkn_w /
 * d_dkn_b (fp32 [head_dim], written, not accumulated).  Any gradient output may be NULL and is then skipped; the norm-gradient
 * pointers must be NULL when the norms are absent.  The probabilities are recomputed (f16 MFMA operands, fp32 accumulation,
 * softmax and dP - D in fp32); d_dout is normalised by one power of two per (batch, head), found on the device, before it is
 * rounded to f16, so gradients far below f16's range keep their precision and an all-zero d_dout gives zeros.  No atomics:
 * bit-identical results run to run. */
int amx_attention_backward(const float* d_q, const float* d_k, const float* d_v, const float* d_qn_w, const float* d_qn_b,
                           const float* d_kn_w, const float* d_kn_b, float norm_eps, const float* d_rope, int n_prefix, int b, int n,
                           int heads, int head_dim, const float* d_out, const float* d_lse, const float* d_dout, float* d_dq, float* d_dk,
                           float* d_dv, float* d_dqn_w, float* d_dqn_b, float* d_dkn_w, float* d_dkn_b, void* d_scratch,
                           size_t scratch_bytes, void* stream);

/* ---- The blocks' linear layers under autograd ---------------------------------------------------------------------------------
 * y = x W^T + b for fp32 d_x [m][k], d_w [n][k], d_bias [n] or NULL, and its gradients: what torch autograd runs as fp32 vendor
 * GEMMs for the seven nn.Linear of an EVA block.  Every operand is rounded ONCE to f16 (x, W, and dy divided by one power of two per
 * call, 2^e <= max |dy| / 8 < 2^(e+1), found on the device; f16 subnormals are kept) and every sum is fp32
 * (v_mfma_f32_16x16x32_f16).  Nothing is cached across calls: the weights are packed per call into d_scratch, the backward
 * re-converts the saved fp32 d_x.  No allocation, no synchronisation (capture-safe); no atomics: bit-identical results run to run.
 *
 * amx_linear_train_scratch_bytes: bytes of d_scratch for either entry (0 outside the envelope: k % 4 == 0, n % 4 == 0, both at most
 * 2^20, m >= 1, m * max(k, n) within int range).  d_x, d_y, d_dy, d_dx, d_dw and d_scratch are 16-byte aligned. */
size_t amx_linear_train_scratch_bytes(long long m, int k, int n);
int amx_linear_forward(const float* d_x, const float* d_w, const float* d_bias, long long m, int k, int n, float* d_y, void* d_scratch,
                       size_t scratch_bytes, void* stream);
/* d_dx [m][k] = dy W, d_dw [n][k] = dy^T x, d_dbias [n] = the fp32 column sums of the UNROUNDED d_dy [m][n] (contiguous); each
 * output is written, not accumulated, and may be NULL: it is then skipped and the others are unchanged bit for bit.  An all-zero
 * d_dy gives exact zeros. */
int amx_linear_backward(const float* d_x, const float* d_w, const float* d_dy, long long m, int k, int n, float* d_dx, float* d_dw,
                        float* d_dbias, void* d_scratch, size_t scratch_bytes, void* stream);

/* ---- The blocks' token LayerNorms and the SwiGLU gate under autograd ---------------------------------------------------------------
 * The row nn.LayerNorm of an EVA block (norm1, attn.norm, norm2, the final norm) and, with d_gate, the SwiGLU product in front of
 * mlp.norm -- what torch autograd runs as F.silu, a multiply and F.layer_norm, each with its own saved tensor
 * (anatomix/model/vit3d/architectures.py:231-260; the blocks are timm's EvaBlock / SwiGLU).  Everything is fp32; d_x, d_gate, d_y,
 * d_dy, d_dx, d_dgate are row-major [m][c], d_w, d_b, d_dw, d_db are [c], d_mean, d_rstd are [m].
 *   u = x, or silu(gate) * x with d_gate;   y = (u - mean) * rstd * w + b   (biased variance, eps inside the root, two-pass statistics)
 * A wave keeps whole rows in registers: a row is read once and u is never stored.  No allocation, no synchronisation (capture-safe);
 * no atomics and a grid that depends on (m, c) alone: bit-identical results run to run.
 *
 * amx_layernorm_train_scratch_bytes: bytes of d_scratch for the backward (per-workgroup partials of dw and db); 0 outside the
 * envelope: c % 4 == 0, 8 <= c <= 4096, m >= 1, m * c < 2^31.  d_x, d_gate, d_w, d_b, d_y, d_dy, d_dx, d_dgate and d_scratch are
 * 16-byte aligned. */
size_t amx_layernorm_train_scratch_bytes(long long m, int c);
int amx_layernorm_train_forward(const float* d_x, const float* d_gate, const float* d_w, const float* d_b, float eps, long long m, int c,
                                float* d_y, float* d_mean, float* d_rstd, void* stream);
/* With x^ = (u - mean) * rstd recomputed from d_x (and d_gate), d_mean and d_rstd, and t = dy * w:
 *   du = rstd * (t - mean_c(t) - x^ * mean_c(t * x^));   d_dw = sum over rows of dy * x^;   d_db = sum over rows of dy
 *   without d_gate: d_dx = du;   with it, s = sigmoid(gate): d_dx = du * gate * s,  d_dgate = du * x * s * (1 + gate * (1 - s))
 * Each output is written, not accumulated, and may be NULL: it is then skipped and the others are unchanged bit for bit. */
int amx_layernorm_backward(const float* d_x, const float* d_gate, const float* d_w, const float* d_mean, const float* d_rstd, const float* d_dy,
                           long long m, int c, float* d_dx, float* d_dgate, float* d_dw, float* d_db, void* d_scratch, size_t scratch_bytes,
                           void* stream);

/* ---- The ViT's conv tokenizer under autograd --------------------------------------------------------------------------------------
 * PatchEmbedDeeper without its 1x1x1 `proj` (deep_tokenizer.py:12-68): stem conv3(1 -> 32) - InstanceNorm - LeakyReLU(0.01) and three
 * stride-2 residual stages 32 -> 32 -> 64 -> 128, one block per level.  Strict precision as in amx_vit_forward: fp32 raw conv outputs,
 * hi + lo f16 operands, three MFMAs per product, fp32 sums; gradient operands are divided by one power of two per tensor, found on the
 * device (2^e <= max / 8 < 2^(e+1)), before they are split.  No float atomics: every long sum is per-workgroup partials in a fixed order,
 * combined in double; results are bit-identical run to run.  No allocation, no synchronisation, no host read-back (capture-safe).
 *
 * Envelope: one input channel, w % 16 == 0, d % 8 == 0, h % 8 == 0, (d / 8)(h / 8)(w / 8) % 64 == 0, n d h w <= 2^22 (two 128^3 views); the byte queries
 * return 0 outside it and the entries refuse it with AMX_ERR_SHAPE before any launch.  params: HOST array of 37 device pointers, fp32,
 * as the torch modules store them: stem conv weight [32][1][3][3][3], bias, norm weight, bias; then per stage conv1 weight, bias, norm1
 * weight, bias, conv2 weight, bias, norm2 weight, bias, skip weight [cout][cin][1][1][1], skip_norm weight, bias.  Every device pointer
 * is 16-byte aligned.
 *
 * amx_tokenizer_train_forward: d_x fp32 [n][1][d][h][w] -> d_h3 fp32 [n][128][d/8][h/8][w/8] (the input of proj), and in d_saved
 * (amx_tokenizer_train_saved_bytes) what the backward reads: per norm the mean and 1 / sqrt(var + eps) per (n, c), the raw conv outputs
 * of the stages, and the hi + lo planes of every activation a conv consumed.  d_saved is state the caller owns until the backward ran;
 * d_scratch (amx_tokenizer_train_scratch_bytes, for either entry) is not: no call reads what an earlier call left there. */
size_t amx_tokenizer_train_saved_bytes(int n, int d, int h, int w);
size_t amx_tokenizer_train_scratch_bytes(int n, int d, int h, int w);
int amx_tokenizer_train_forward(const float* d_x, const float* const* params, int n, int d, int h, int w, float in_eps, float* d_h3,
                                void* d_saved, size_t saved_bytes, void* d_scratch, size_t scratch_bytes, void* stream);
/* From d_dh3 [n][128][d/8][h/8][w/8] (contiguous): grads, a HOST array of 37 device pointers in the order of params.  Every output is
 * written, not accumulated, and may be NULL: it is then skipped and the others are unchanged bit for bit.  The seven conv biases feed
 * an InstanceNorm, which removes them: their gradients are exact zeros.  There is no gradient for d_x. */
int amx_tokenizer_backward(const float* d_dh3, const float* d_x, const float* const* params, const void* d_saved, int n, int d, int h, int w,
                           float in_eps, float* const* grads, void* d_scratch, size_t scratch_bytes, void* stream);
/* Test aids.  _export: the saved activation of `site` 0 .. 6 (h0, a1 of stage 0, h1, a1 of stage 1, h2, a1 of stage 2, h3) as fp32
 * [n][c][..] (the sum of its hi and lo planes); synchronises the device before and after.  _route: the kernel instances one forward
 * and one backward launch at this shape, one name per line, in launch order, without launching anything. */
int amx_tokenizer_train_export(const void* d_saved, int n, int d, int h, int w, int site, float* d_out);
int amx_tokenizer_train_route(int n, int d, int h, int w, char* buf, size_t cap);

/* ---- The ViT's patch decoder on sampled rows, under autograd --------------------------------------------------------------------
 * Contrastive pretraining of the ViT is single-scale NCE on the decoded volume (pretraining/models/supcl_model.py:403-410,
 * nce_layers = [-1]) and PatchSampleF reads num_patches voxels of it per view (pretraining_networks.py:472-480).  These entries
 * replace the dense PatchDecode (three ConvTranspose3d(k = 2, s = 2), channel LayerNorm + erf-GELU between them; the up_projection of
 * anatomix/model/vit3d/architectures.py:231-260), the per-voxel output norms (architectures.py:36-52, 55-86), that gather, and what
 * torch autograd replays for them -- for the sampled voxels only.  Kernel == stride, so voxel (z, y, x) is a three-layer MLP on token
 * t = ((z >> 3) grid_h + (y >> 3)) grid_w + (x >> 3): stage s = 1, 2, 3 applies W_s[:, :, kz, ky, kx] with (kz, ky, kx) = bit (3 - s)
 * of (z, y, x).
 *
 * d_tokens: fp32 [n][grid_d grid_h grid_w][e], the tokens after the final norm without the register tokens.  d_coords: int64 [p][3]
 * as (z, y, x), shared by the n views; any value is clamped into the volume.  params: HOST array of 12 device pointers, fp32, as the
 * torch modules store them: {W1 [e][c1][2][2][2], b1, ln1 weight, ln1 bias, W2 [c1][c2][2][2][2], b2, ln2 weight, ln2 bias,
 * W3 [c2][c][2][2][2], b3, output-norm weight, output-norm bias}; the conv biases may be NULL, the last two are read for
 * out_norm == 2 only.  out_norm: 0 none, 1 layernorm (no affine), 2 layernorm_affine, with out_eps; ln_eps: the decoder norms'.
 * d_rows: fp32 [n][p][c].  All arithmetic is fp32; no atomics, every sum in one fixed order: bit-identical results run to run.  No
 * allocation, no synchronisation, no host read-back (capture-safe).
 *
 * amx_vit_decode_rows_scratch_bytes: bytes of d_scratch (16-byte aligned) for either entry; 0 outside the envelope (e, c1, c2 in
 * 1 .. 1056, c in 1 .. 64, n in 1 .. 65535, n p <= 2^20), which the entries refuse with AMX_ERR_SHAPE. */
size_t amx_vit_decode_rows_scratch_bytes(int n, int p, int e, int c1, int c2, int c);
int amx_vit_decode_rows_forward(const float* d_tokens, const long long* d_coords, const void* const* params, int n, int p, int grid_d,
                                int grid_h, int grid_w, int e, int c1, int c2, int c, float ln_eps, int out_norm, float out_eps,
                                float* d_rows, void* d_scratch, size_t scratch_bytes, void* stream);
/* From d_drows [n][p][c]: d_dtokens [n][tokens][e] (exact zeros where no row points) and grads, a HOST array of 12 device pointers in
 * the order of params.  Every output is written, not accumulated, and may be NULL: it is then skipped and the others are unchanged
 * bit for bit.  The weight slices of offsets no row selects get exact zeros.  The forward's passes are re-run into d_scratch: the
 * call reads nothing an earlier call left there. */
int amx_vit_decode_rows_backward(const float* d_tokens, const long long* d_coords, const void* const* params, int n, int p, int grid_d,
                                 int grid_h, int grid_w, int e, int c1, int c2, int c, float ln_eps, int out_norm, float out_eps,
                                 const float* d_drows, float* d_dtokens, void* const* grads, void* d_scratch, size_t scratch_bytes,
                                 void* stream);

/* ---- The ViT's patch decoder on the whole volume, with the spatial output norms, under autograd -------------------------------------
 * Replaces, for training, the dense PatchDecode (the up_projection of anatomix/model/vit3d/architectures.py:231-260: three
 * ConvTranspose3d(k = 2, s = 2), channel LayerNorm + erf-GELU between them), the output norms that need the whole volume
 * (architectures.py:28-33 ChannelDemean, architectures.py:55-86 nn.InstanceNorm3d(affine=False)) and what torch autograd replays for
 * them: the path of a contrastive step whose output norm is spatial (pretraining/models/supcl_model.py:403-410) and of dense
 * supervision on the ViT's features.  A stage is a row product [R, Cin] x [Cin, 8 Cout]; the rows stay in nested order (token, then
 * the child offset of stage 1, then of stage 2), so a stage's output is the next one's input without moving data; only the last
 * stage stores planar.
 *
 * d_tokens: fp32 [n][grid_d grid_h grid_w][e], the tokens after the final norm without the register tokens.  params: HOST array of 10
 * device pointers, fp32, as the torch modules store them: {W1 [e][c1][2][2][2], b1, ln1 weight, ln1 bias, W2 [c1][c2][2][2][2], b2,
 * ln2 weight, ln2 bias, W3 [c2][c][2][2][2], b3}; the conv biases may be NULL.  out_norm: 0 none, 1 demean (per (n, c): subtract the
 * spatial mean), 2 instance ((x - mean) / sqrt(biased var + out_eps) per (n, c)); ln_eps: the decoder norms'.  d_out: fp32
 * [n][c][8 grid_d][8 grid_h][8 grid_w].  Products run on the f32-input MFMA (exact fp32 products, fp32 sums); LayerNorm, GELU, their
 * adjoints and every reduction are fp32, the per-(n, c) statistics are combined in double.  No atomics, every long sum through partials
 * added in one fixed order: bit-identical results run to run.  No allocation, no synchronisation, no host read-back (capture-safe).
 *
 * d_saved (amx_vit_decoder_train_saved_bytes) is state the caller owns until the backward ran: the raw stage outputs a_1, a_2, the
 * mean and rstd of their rows, the output norm's mean and rstd per (n, c).  d_scratch (amx_vit_decoder_train_scratch_bytes, for either
 * entry) is not: no call reads what an earlier call left there.  Both sizes are 0 outside the envelope -- e, c1, c2 multiples of 4 up
 * to 1056 / 328 / 104, c in 1 .. 128, any token grid with extents >= 1, n c <= 65535, every tensor below 2^31 elements -- which the
 * entries refuse with AMX_ERR_SHAPE.  Both buffers are 16-byte aligned. */
size_t amx_vit_decoder_train_saved_bytes(int n, int grid_d, int grid_h, int grid_w, int e, int c1, int c2, int c);
size_t amx_vit_decoder_train_scratch_bytes(int n, int grid_d, int grid_h, int grid_w, int e, int c1, int c2, int c);
int amx_vit_decoder_train_forward(const float* d_tokens, const void* const* params, int n, int grid_d, int grid_h, int grid_w, int e, int c1,
                                  int c2, int c, float ln_eps, int out_norm, float out_eps, float* d_out, void* d_saved, size_t saved_bytes,
                                  void* d_scratch, size_t scratch_bytes, void* stream);
/* From d_dout (the gradient of d_out, contiguous) and, for out_norm == 2, d_out itself (else it may be NULL): d_dtokens
 * [n][tokens][e] and grads, a HOST array of 10 device pointers in the order of params.  Every output is written, not accumulated, and
 * may be NULL: it is then skipped and the others are unchanged bit for bit.  h_1, h_2 are recomputed from d_saved. */
int amx_vit_decoder_backward(const float* d_dout, const float* d_out, const float* d_tokens, const void* const* params, const void* d_saved,
                             size_t saved_bytes, int n, int grid_d, int grid_h, int grid_w, int e, int c1, int c2, int c, float ln_eps,
                             int out_norm, float out_eps, float* d_dtokens, void* const* grads, void* d_scratch, size_t scratch_bytes,
                             void* stream);

/* ---- The whole 3D ViT variant `anatomix-dev-vit` (PrimusV2-S) as one forward ------------------------------------------------
 * Replaces PrimusV2.forward (anatomix/model/vit3d/architectures.py:231-260 with the wrapper's extensions :89-165, tokenizer
 * deep_tokenizer.py:12-68, registry entry load_from_hf.py:25-35): conv tokenizer (stem + three stride-2 residual stages + 1x1x1
 * projection), position embedding + register tokens, `depth` EVA blocks (LayerNorm, q/k/v, per-head QK LayerNorm + rotary
 * embedding + softmax attention, inner LayerNorm, output projection, LayerScale; SwiGLU MLP with sub-LayerNorm), final LayerNorm,
 * patch decoder (three ConvTranspose3d(k = 2, s = 2) with channel LayerNorm + GELU between them), ChannelDemean.  Every kernel is
 * this library's (amx_tokenizer.hip, amx_gemm.hip, amx_attention.hip); none of it calls a vendor GEMM / conv library.
 * The blocks themselves live in third-party packages absent from this image: arithmetic follows oracle/vit_ref.py's restatement
 * (PARITY WITH THE UPSTREAM PACKAGE UNPINNED). */
typedef struct amx_vit_cfg {
  int32_t input_channels;       /* 1 */
  int32_t num_classes;          /* output channels, a multiple of 4 */
  int32_t embed_dim;            /* architectures.py:20-25 (PRIMUS_CONFIGS: 396 / 792 / 864 / 1056), a multiple of 4, <= 1280 */
  int32_t depth;                /* eva_depth */
  int32_t heads;                /* eva_numheads; head_dim = embed_dim / heads even, <= 80 */
  int32_t num_register_tokens;  /* architectures.py:117-120 */
  int32_t grid_d, grid_h, grid_w; /* token grid = input_shape / 8 */
  int32_t hidden;               /* SwiGLU hidden width (int(embed_dim * 4 * 2 / 3)), 16 .. 3072 (a multiple of 4 above 1088) */
  int32_t dec1, dec2;           /* channel widths after the first / second transposed conv (oracle/vit_ref.py::vit_plan) */
  int32_t qk_norm;              /* architectures.py:108-115 */
  int32_t scale_attn_inner;     /* LayerNorm between attention and its output projection */
  int32_t layer_scale;          /* gamma_1 / gamma_2 present (init_values is not None) */
  float in_eps;                 /* tokenizer InstanceNorm epsilon (deep_tokenizer.py:66-68) */
  int32_t out_norm;             /* 0 none, 1 ChannelDemean (architectures.py:28-33); other modes are applied by the caller */
  int32_t decoder_split;        /* 1: hi + lo f16 operands in the decoder (fp32-grade), 0: plain f16 */
  int32_t stem_split;           /* 1: the stem's output (the largest tensor) keeps its lo plane; 0: single f16 -- half the bytes of the
                                 * two kernels that touch it, +3.7e-4 rel-L2 on the output (measured) */
} amx_vit_cfg;
typedef struct amx_vit amx_vit_t;

int amx_vit_create(amx_vit_t** out, const amx_vit_cfg* cfg);
void amx_vit_destroy(amx_vit_t* h);
/* Parameter slots: amx_vit_param_name(h, i) is the state_dict key (anatomix_amd.model.vit3d.PrimusV2) of slot i. */
int amx_vit_num_params(const amx_vit_t* h);
const char* amx_vit_param_name(const amx_vit_t* h, int idx);
/* d_params[i]: contiguous fp32 device tensor of slot i; d_rope: fp32 [grid tokens][2 * head_dim] = per token [sin | cos].
 * Packs / copies everything into library-owned memory (call again after the parameters change). */
int amx_vit_load(amx_vit_t* h, const float* const* d_params, int count, const float* d_rope, void* stream);
size_t amx_vit_workspace_bytes(const amx_vit_t* h, int n);
/* d_x: fp32 [n][1][8 grid_d][8 grid_h][8 grid_w]; d_y: fp32 [n][num_classes][same volume].  d_ws: amx_vit_workspace_bytes(h, n)
 * bytes, 256-byte aligned.  n_blocks < 0: all blocks (a smaller count is a debugging aid). */
int amx_vit_forward(amx_vit_t* h, const float* d_x, float* d_y, int n, void* d_ws, size_t ws_bytes, int n_blocks, void* stream);

/* amx_vit_forward with taps (test aid; the stage-by-stage walk of tests/_vit_walk.py).  The workspace regions of tokenizer, blocks and
 * decoder alias each other and the token stream is updated in place, so an intermediate can only be read while the forward runs: for every
 * request, the named buffer is copied to d_dst (`bytes` = its capacity) by a device-to-device copy enqueued on `stream` right after the
 * launch that produces it, and `route` receives that launch's instance name (e.g. wsgemm<2,5,4,RESID,f16,4w>, tokconv<27,2,2,4,split>,
 * ln_rows_vec<f32,2>).  d_dst NULL: the route only.  No launch is added, moved or routed differently: d_y has the bits of amx_vit_forward.
 * Names (k = 0..2 tokenizer stage, b = block; "x | y" = two ranges back to back, each half of amx_vit_tap_bytes):
 *   h0, p0                 stem output and its 2x2x2 average: f16 channels-last [n][D][H][W][32], hi | lo (hi alone when stem_split == 0)
 *   s{k}.raw1 .raw2 .raws  fp32 channels-last conv outputs (conv1, conv2, skip);  s{k}.ss1 .ss2 .sss  InstanceNorm scale | shift, fp32 [n][C]
 *   s{k}.a1, s{k}.h, s{k}.p   f16 hi | lo: activation behind conv1, stage output, its average (no s2.p)
 *   tokens                 fp32 [n][T][E] behind the tokenizer (registers in front)
 *   b{b}.ln1 .ln_attn .ln2 f16 [n T][Ep] operand rows;  b{b}.attn fp32 [n T][E];  b{b}.tok1 .tok2 fp32 [n T][E] token stream
 *   b{b}.hd                f16 [n T][hidden up to 16];  b{b}.ln_mlp f16 [n T][hidden up to 32]
 *   d.ln, d1.in, d2.in     f16 hi | lo decoder operand rows [rows][channels up to 32] (hi alone when decoder_split == 0)
 *   d0.raw, d1.raw         fp32 [8 rows][C] -- absent when the stage's LayerNorm + GELU is fused into the product (Cp == 128)
 *   d.mean                 fp32 [n][num_classes] (out_norm == 1);  y  the output itself
 * Unknown names (or a block >= n_blocks) fail with AMX_ERR_INVALID, short buffers with AMX_ERR_WORKSPACE, before the first launch. */
typedef struct amx_vit_tap {
  const char* name;
  void* d_dst;       /* device buffer, or NULL */
  size_t bytes;      /* its capacity */
  char route[160];   /* out: the producing launch */
} amx_vit_tap;
size_t amx_vit_tap_bytes(const amx_vit_t* h, int n, const char* name);   /* 0 for an unknown name */
int amx_vit_forward_taps(amx_vit_t* h, const float* d_x, float* d_y, int n, void* d_ws, size_t ws_bytes, int n_blocks, amx_vit_tap* taps,
                         int n_taps, void* stream);

/* ---- the ViT under sliding_window_inference (convex_adam_utils.py:202-219 / train_segmentation.py:194-199; the reference
 * presents anatomix-dev-vit as "Requires 128^3 inputs, but amenable to sliding window").  The roi is the handle's input shape,
 * 8 * grid, on every entry below. */

/* Bytes of workspace amx_vit_forward_windows needs for n_windows (1 .. 16) windows: the gathered single-channel windows and the
 * forward's own workspace.  0 for a null handle or a count out of range. */
size_t amx_vit_windows_workspace_bytes(const amx_vit_t* h, int n_windows);

/* One batch of windows of a resident volume, as sliding_window_inference hands sw_batch_size windows to the predictor and blends
 * the predictions (convex_adam_utils.py:202-219 / train_segmentation.py:194-199): the n_windows (1 .. 16) roi-sized windows at
 * the host array offsets_zyx [n_windows][3] are cut from d_vol fp32 [vd][vh][vw] (single channel) by a gather kernel, run as one
 * batch through the tokenizer, blocks and decoder of amx_vit_forward, and the last decoder product runs once per window, in
 * window order on `stream`, with an accumulating epilogue:
 *   d_acc[c][oz + z][oy + y][ox + x] += d_wmap[z][y][x] * (value + bias[c] - mean[window][c])
 * d_acc fp32 [num_classes][vd][vh][vw], d_wmap fp32 [roi].  ChannelDemean (out_norm == 1) stays per window.  No [n][C][roi]
 * output tensor exists on this route.  Every (channel, voxel) of a window has one owner: plain load-add-store, no atomics,
 * results bit-identical from run to run; rows take 16-byte accesses when ox, vw and the bases allow it and scalar ones otherwise,
 * with identical values.  Every check comes before the first launch: null arguments (AMX_ERR_INVALID), a handle that is not
 * loaded (AMX_ERR_NOT_LOADED), n_windows out of range (AMX_ERR_INVALID), a volume smaller than the roi or a window outside the
 * volume (AMX_ERR_SHAPE; padding is the caller's), a workspace below amx_vit_windows_workspace_bytes(h, n_windows) or not
 * 256-byte aligned (AMX_ERR_WORKSPACE). */
int amx_vit_forward_windows(amx_vit_t* h, const float* d_vol, int vd, int vh, int vw, int n_windows, const int* offsets_zyx,
                            const float* d_wmap, float* d_acc, void* d_ws, size_t ws_bytes, void* stream);

/* Bytes of workspace amx_vit_sliding_window needs for batches of n_batch (1 .. 16) windows (the sw_batch_size of
 * convex_adam_utils.py:202-219 / train_segmentation.py:194-199): one batch is in flight at a time. */
size_t amx_vit_sliding_window_workspace_bytes(const amx_vit_t* h, int n_batch);

/* sliding_window_inference(volume, roi, n_batch, vit, overlap, mode, sigma_scale) in one call (convex_adam_utils.py:202-219;
 * with a head, train_segmentation.py:194-199): amx_sliding_window's contract with the roi implied by the handle.  The call zeroes
 * d_acc fp32 [num_classes][vd*vh*vw], builds the window weights with amx_sw_importance_map's kernel (cached on the handle per
 * mode and sigma_scale; the first call allocates them), writes d_cnt fp32 [vd*vh*vw] with amx_sw_count_all, runs the windows of
 * amx_sw_plan in batches of n_batch through amx_vit_forward_windows and ends with amx_sw_finish(out_kind, ...): features in
 * d_acc, or logits / labels in d_out (d_w, d_b, classes: the head, NULL / 0 for features).  Everything runs on `stream`, one
 * batch at a time; no host synchronisation.  While `stream` is capturing the call is refused (AMX_ERR_INVALID).  Every check
 * comes before the first launch and a refused call leaves all buffers untouched: those of amx_vit_forward_windows (with n_batch
 * for n_windows), overlap / mode / sigma_scale as for amx_sliding_window, the head as for amx_sw_finish. */
int amx_vit_sliding_window(amx_vit_t* h, const float* d_vol, int vd, int vh, int vw, double overlap, int mode, double sigma_scale,
                           int n_batch, int out_kind, const float* d_w, const float* d_b, int classes, float* d_acc, float* d_cnt,
                           void* d_out, void* d_ws, size_t ws_bytes, void* stream);
/* y[m][n] = sum_k x[m][k] w[n][k] + b[n] through the ViT's MFMA product kernel (f16 operands, or hi + lo pairs when split != 0):
 * a test entry for nn.Linear-shaped products; synchronous (allocates and frees its operand buffers). */
int amx_linear(const float* d_x, const float* d_w, const float* d_b, int m, int k, int n, int split, float* d_y, void* stream);

/* SupPatchNCELoss.forward + its backward (pretraining/models/supcl_model.py:73-226) for one nce layer.
 * d_feat: fp32 [n][c], n = views * patches anchors in (view, patch) order (features.view(ntps * num_patches, nc),
 * supcl_model.py:134); d_labels: int32 [n], the segmentation class of every anchor (the label gather of :100-112,
 * tiled over the views); flags = opt.weigh_rarity / opt.balance_denominator / (opt.weighting_mode == 'sqrt');
 * d_loss: 1 float; d_grad: fp32 [n][c] = d loss / d feat, or NULL for the forward only.
 * d_scratch: amx_supcon_scratch_bytes(n, c) bytes.  Deterministic (fixed-order reductions). */
size_t amx_supcon_scratch_bytes(int n, int c);
int amx_supcon_loss(const float* d_feat, const int* d_labels, int n, int c, float temperature, int weigh_rarity,
                    int balance_denominator, int sqrt_mode, float* d_loss, float* d_grad, void* d_scratch,
                    size_t scratch_bytes, void* stream);

/* Projection head of PatchSampleF (pretraining/models/pretraining_networks.py:338-350, applied at :505-511) in train
 * mode: n_layers x [Linear(bias=False) -> BatchNorm1d(batch statistics) -> activation], no activation after the last
 * layer, affine parameters optional per layer.  All device tensors fp32, row-major:
 *   d_x [n][cin] the sampled features; w[l] [width][cin or width]; gamma[l] / beta[l] [width] or NULL (affine=False);
 *   running_mean[l] / running_var[l] [width] updated in place like nn.BatchNorm1d (momentum, unbiased variance) or NULL;
 *   d_z, d_y [n_layers][n][width]: pre-norm and post-activation outputs of every layer (kept for the backward;
 *   the head's output is d_y + (n_layers - 1) * n * width); d_mean, d_rstd [n_layers][width] the batch statistics.
 * w, gamma, beta, running_mean, running_var are HOST arrays of n_layers device pointers.
 * Limits: 1 <= n <= 2048, cin % 4 == 0, width % 8 == 0, 1 <= n_layers <= 8.  Two kernels per layer. */
int amx_mlp_head_forward(const float* d_x, int n, int cin, int width, int n_layers, const float* const* w,
                         const float* const* gamma, const float* const* beta, float* const* running_mean,
                         float* const* running_var, float eps, float momentum, int act, float slope, float* d_z, float* d_y,
                         float* d_mean, float* d_rstd, void* stream);

/* Backward of amx_mlp_head_forward: d_dy [n][width] = d loss / d head output.  Writes dw[l] (shape of w[l]), dgamma[l] /
 * dbeta[l] (where gamma[l] is not NULL) and d_dx [n][cin] (nullable).  d_scratch: amx_mlp_head_scratch_bytes(n, cin, width).
 * Four small kernels per layer; deterministic (fixed-order reductions). */
size_t amx_mlp_head_scratch_bytes(int n, int cin, int width);
int amx_mlp_head_backward(const float* d_dy, const float* d_x, int n, int cin, int width, int n_layers,
                          const float* const* w, const float* const* gamma, int act, float slope, const float* d_z,
                          const float* d_y, const float* d_mean, const float* d_rstd, float* const* dw, float* const* dgamma,
                          float* const* dbeta, float* d_dx, void* d_scratch, size_t scratch_bytes, void* stream);

/* Backward of a k3 reflect convolution whose output gradient is nonzero only at p sampled voxels per sample -- the contrastive step
 * taps the output conv (module 65) at 512 voxels and nothing else reads the network's output (supcl_model.py:801-843): d_grows fp32
 * [n][p][cout] at d_coords int64 [p][3]; d_x the conv's 16-bit channels-last input [n][d][h][w][x_channels]; d_w fp32
 * [cout][cin][27].  d_dw fp32 [cout][cin][27] is written; d_din (optional) is a ZERO-FILLED 16-bit [n][d][h][w][din_channels] tensor
 * that receives the data gradient at the <= 27 p voxels per sample it is nonzero at.  Same rounding points as scatter_rows + the dense
 * weight / data gradient (rows rounded to the storage type, 16-bit weights in the data gradient, fp32 sums, one rounding), fixed
 * summation order.  cout, cin <= 16.  d_scratch: amx_conv3d_backward_sampled_scratch_bytes(p) bytes (neighbour masks of the samples,
 * partial weight-gradient sums). */
size_t amx_conv3d_backward_sampled_scratch_bytes(int p);
int amx_conv3d_backward_sampled(const float* d_grows, const long long* d_coords, const void* d_x, int x_channels, const float* d_w, int n,
                                int p, int d, int hh, int w, int cout, int cin, float* d_dw, void* d_din, int din_channels, void* d_scratch,
                                size_t scratch_bytes, int precision, void* stream);

/* The heads and losses of ONE contrastive step as batches (supcl_model.py:801-843 walks the nce layers one by one; the chains are
 * independent and identical in structure).  A replayed HIP graph pays per DEPENDENT node, not per byte: n_heads chains of ~30 small
 * launches each become one chain whose every launch serves all heads (<= 8; same rows n, same width, same depth; own input widths
 * cin[h]).  Arrays over (head, layer) are flattened [h * n_layers + l]; d_z / d_y / d_mean / d_rstd / d_scratch are per head with
 * the single-head layouts and sizes above.  Per head the arithmetic and its order are those of amx_mlp_head_forward / _backward:
 * bit-identical results.  amx_supcon_loss_batch: n_losses problems of one shape [n][c] (scratch: n_losses slices of
 * amx_supcon_scratch_bytes(n, c); d_grad NULL: losses only); amx_gather_labels_batch: the class ids of n_maps feature maps of sizes
 * dims[3 m ..] = (d, h, w) from one segmentation. */
int amx_mlp_heads_forward(int n_heads, const float* const* d_x, int n, const int* cin, int width, int n_layers, const float* const* w,
                          const float* const* gamma, const float* const* beta, float* const* running_mean, float* const* running_var,
                          float eps, float momentum, int act, float slope, float* const* d_z, float* const* d_y, float* const* d_mean,
                          float* const* d_rstd, void* stream);
int amx_mlp_heads_backward(int n_heads, const float* const* d_dy, const float* const* d_x, int n, const int* cin, int width, int n_layers,
                           const float* const* w, const float* const* gamma, int act, float slope, const float* const* d_z,
                           const float* const* d_y, const float* const* d_mean, const float* const* d_rstd, float* const* dw,
                           float* const* dgamma, float* const* dbeta, float* const* d_dx, void* const* d_scratch, size_t scratch_bytes,
                           void* stream);
int amx_supcon_loss_batch(int n_losses, const float* const* d_feat, const int* const* d_labels, int n, int c, float temperature,
                          int weigh_rarity, int balance_denominator, int sqrt_mode, float* const* d_loss, float* const* d_grad,
                          void* d_scratch, size_t scratch_bytes, void* stream);
int amx_gather_labels_batch(const float* d_seg, int sd, int sh, int sw, int n_maps, const long long* const* d_coords, int p, const int* dims,
                            int views, int* const* d_labels, void* stream);

/* Patch coordinates of PatchSampleF's no-mask branch (pretraining_networks.py:443-470: `randperm(n_voxels)[:num]`, then the
 * flat ids unravelled): d_draws int64 [n_draws], values in [0, d0*d1*d2) drawn WITH replacement by the caller's generator;
 * d_coords int64 [num][3] receives the C-order coordinates of the first `num` distinct draws in draw order -- the same
 * distribution as a random permutation's head, without sorting every voxel.  num <= n_draws <= 4096.  One launch. */
/* Sampled feature taps of the contrastive step (pretraining_networks.py:472-480 gathers feat[:, :, x, y, z] at num_patches
 * coordinates): rows[n][p][c] (fp32) = src[n][coords[p]][c] read in place -- src a 16-bit channels-last tensor (dtype = AMX_PREC_F16 /
 * AMX_PREC_BF16) or an fp32 tensor (dtype 2, e.g. the NCDHW network output), ELEMENT strides -- and its adjoint
 * dst[n][coords[p]][c] (= or +=) rows[n][p][c] into a 16-bit channels-last tensor (BYTE strides; fp32 add, one rounding; coords must
 * be distinct).  d_coords: int64 [p][3] = (z, y, x). */
int amx_gather_rows(const void* d_src, int dtype, long long src_sn, long long src_sz, long long src_sy, long long src_sx, long long src_sc,
                    const long long* d_coords, int n, int p, int c, float* d_rows, void* stream);
int amx_scatter_rows(const float* d_rows, const long long* d_coords, void* d_dst, int precision, long long dst_sn, long long dst_sz,
                     long long dst_sy, long long dst_sx, int n, int p, int c, int accumulate, void* stream);

int amx_sample_coords(const long long* d_draws, int n_draws, int num, int d0, int d1, int d2, long long* d_coords, void* stream);
/* The same branch on a SMALL grid (d0 d1 d2 <= 4096 voxels, e.g. 512 patches from an 8^3 map = all of it): d_keys holds one random
 * non-negative 64-bit key per voxel (torch.randint: torch's generator seeds it); the voxels are ordered by key (ties by index) in one
 * launch and the first `num` are unravelled to d_coords [num][3] -- a uniformly random permutation prefix, replacing
 * torch.randperm(n)[:num] (pretraining_networks.py:443-470) and its dozen small launches. */
int amx_sample_perm(const long long* d_keys, int d0, int d1, int d2, int num, long long* d_coords, void* stream);
/* Class ids of the sampled patches for SupPatchNCELoss (supcl_model.py:100-123: F.interpolate(seg, size = the feature map, mode =
 * 'nearest') gathered at the patch coordinates): d_seg fp32 [sd][sh][sw] (one label map shared by the views), d_coords int64
 * [p][3] in the (d, hh, w) grid of the feature map -> d_labels int32 [views][p] (round to nearest, tiled over the views). */
int amx_gather_labels(const float* d_seg, int sd, int sh, int sw, const long long* d_coords, int p, int d, int hh, int w, int views,
                      int* d_labels, void* stream);

/* The optimizer step of the contrastive step: torch.optim.AdamW as the reference builds it for netG and netF
 * (pretraining/models/supcl_model.py:510-516, 584-590; stepped at :628-661), every parameter tensor of one optimizer in ONE
 * launch per 48 tensors.  `tensors` is a HOST array; every pointer in it is a device pointer to contiguous fp32 (step: one fp32
 * scalar holding the step count t AFTER this step's increment -- torch's capturable state layout, so the call can be captured
 * in a HIP graph and a state_dict moves between this and torch.optim.AdamW).  In place:
 *   p *= 1 - lr wd;  m += (g - m)(1 - beta1);  v = v beta2 + (1 - beta2) g g;
 *   p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)            (maximize: g -> -g).  amsgrad is not offered.
 * The hyper-parameters are doubles because torch holds them as Python floats: 1 - beta2, 1 - lr wd and the bias corrections are
 * formed in double and rounded once (1 - 0.999f differs from (float)(1 - 0.999) by 1.3e-5). */
typedef struct {
  void* param;
  const void* grad;
  void* exp_avg;
  void* exp_avg_sq;
  const void* step;
  long long numel;
} amx_adamw_tensor;
int amx_adamw_step(const amx_adamw_tensor* tensors, int count, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int maximize, void* stream);
/* The same step with the hyper-parameters READ FROM THE DEVICE when the kernel runs: d_hyper = five doubles {lr, beta1, beta2, eps,
 * weight_decay}.  By-value arguments are frozen into a captured HIP graph; the reference changes lr every epoch through its
 * schedulers (pretraining/models/base_model.py: update_learning_rate / get_scheduler), so a graph-replayed step takes them from a
 * buffer that a captured host-to-device copy refreshes (anatomix_amd/pretraining/optim.py).  Values are not range-checked here. */
int amx_adamw_step_dev(const amx_adamw_tensor* tensors, int count, const double* d_hyper, int maximize, void* stream);
/* amx_adamw_step_dev with gradient clipping folded into the read of the gradients (supcl_model.py:631-655: clip_grad_norm_ between
 * unscale_ and the step): the kernel reads the group's total norm from d_total_norm (one fp32 on the device, e.g. written by
 * amx_grad_norms), forms coef = min(max_norm / (norm + 1e-6), 1) in fp32 as torch.nn.utils.clip_grad_norm_ does, and uses
 * g * coef -- rounded to fp32 on its own, like torch's separate multiply -- in place of g.  The gradients themselves are NOT
 * modified.  max_norm = inf reproduces amx_adamw_step_dev bit for bit. */
int amx_adamw_step_clip_dev(const amx_adamw_tensor* tensors, int count, const double* d_hyper, int maximize, const float* d_total_norm,
                            double max_norm, void* stream);
/* L2 norms of `groups` lists of contiguous fp32 device tensors (netG's gradients, netF's gradients) in one call: `tensors` is
 * a HOST array, `group` in [0, groups) says which list a tensor belongs to; d_out = float[groups] on the device (0 for a group
 * without tensors; an inf / NaN reaches the norm of its own group only).  Deterministic: per-block partial sums of squares in
 * d_scratch (amx_grad_norms_scratch_bytes of the same table; never 0, 0 = invalid table) and a fixed-order reduction in a second
 * small launch, no atomics; at most 21 sequential fp32 additions, double from there on.  Does not synchronise; capturable. */
typedef struct {
  const void* grad;
  long long numel;
  long long group;
} amx_grad_tensor;
size_t amx_grad_norms_scratch_bytes(const amx_grad_tensor* tensors, int count, int groups);
int amx_grad_norms(const amx_grad_tensor* tensors, int count, int groups, float* d_out, void* d_scratch, size_t scratch_bytes,
                   void* stream);

/* ---- registration feature post-processing (what the reference does to the extracted features before the convex
 * optimisation; all fp32, planar [C][H][W][D] device tensors, batch 1 as everywhere in that pipeline) ---- */

/* MINDSSC(img, radius, dilation) (anatomix/registration/convex_adam_utils.py:311-406): d_img fp32 [H][W][D] ->
 * d_out fp32 [12][H][W][D], channels in the reference's final (permuted) order.  radius in {1, 2}, dilation in [1, 4].
 * d_scratch: amx_mindssc_scratch_bytes(H, W, D).  The global mean the descriptor variance is clamped against
 * (`mind_var.mean().item()`, :389-393) stays on the device: no host synchronisation. */
size_t amx_mindssc_scratch_bytes(int H, int W, int D);
int amx_mindssc(const float* d_img, int H, int W, int D, int radius, int dilation, float* d_out, void* d_scratch,
                size_t scratch_bytes, void* stream);

/* F.avg_pool3d(cat(scale_a * a, scale_b * b), g, stride=g) in one pass: the `pred * downscale_feat_scalar`,
 * merge_features' concat (instance_optimization.py:111-117) and the grid_sp pooling of
 * run_convex_adam_with_network_feats.py:164-205.  d_a fp32 [ca][H][W][D] (may be NULL with ca == 0), d_b [cb][H][W][D];
 * d_out [ca + cb][H/g][W/g][D/g] (floor division like avg_pool3d). */
int amx_avg_pool3d_cat(const float* d_a, int ca, float scale_a, const float* d_b, int cb, float scale_b, int H, int W, int D,
                       int g, float* d_out, void* stream);

/* One pass of apply_avg_pool3d (convex_adam_utils.py:105-131): F.avg_pool3d(x, k, padding=k/2, stride=1), zero padding
 * counted in the divisor.  d_in, d_out fp32 [c][H][W][D], distinct buffers; k odd, 3 <= k <= 9. */
int amx_box_filter3d(const float* d_in, float* d_out, int c, int H, int W, int D, int k, void* stream);

/* correlate(mind_fix, mind_mov, disp_hw, ...) (convex_adam_utils.py:409-491): d_fix, d_mov fp32 [c][h][w][d] (the pooled
 * features) -> d_ssd fp32 [(2 disp_hw + 1)^3][h][w][d] (twice box-filtered sum of squared differences, displacement
 * index (dx * k + dy) * k + dz as the reference's view/transpose/reshape leaves it) and d_argmin int64 [h][w][d]
 * (nullable).  disp_hw in {1, 2, 3}.  d_scratch: amx_correlate_scratch_bytes(h, w, d, disp_hw). */
size_t amx_correlate_scratch_bytes(int h, int w, int d, int disp_hw);
int amx_correlate_ssd(const float* d_fix, const float* d_mov, int c, int h, int w, int d, int disp_hw, float* d_ssd,
                      long long* d_argmin, void* d_scratch, size_t scratch_bytes, void* stream);

/* ---- registration stage 1: the discrete solver downstream of amx_correlate_ssd (csrc/amx_regsolve.hip; fp32, planar
 * [C][h][w][d], batch 1).  Every entry validates its arguments and returns an error without launching anything. ---- */

/* coupled_convex (convex_adam_utils.py:494-552): d_ssd [(2 disp_hw + 1)^3][h][w][d] as amx_correlate_ssd leaves it,
 * d_argmin int64 [h][w][d] (nullable: recomputed from d_ssd) -> d_disp_soft [3][h][w][d] in grid units; channel c is the
 * mesh component (m % k, (m / k) % k, m / k^2)[c] - disp_hw of label m.  The penalty accumulates over the six iterations
 * as in the reference, but d_ssd is NOT modified (the reference writes the coupled cost through a view into its ssd).
 * Two launches per iteration.  d_scratch: amx_coupled_convex_scratch_bytes(h, w, d). */
size_t amx_coupled_convex_scratch_bytes(int h, int w, int d);
int amx_coupled_convex(const float* d_ssd, const long long* d_argmin, int h, int w, int d, int disp_hw, float* d_disp_soft,
                       void* d_scratch, size_t scratch_bytes, void* stream);

/* One iteration j in [0, 6] of the above from given state: d_soft_hist [j][3][h][w][d] are the soft fields s_0 .. s_{j-1}
 * (nullable for j == 0, the plain argmin of d_ssd) -> d_soft_out [3][h][w][d] = s_j and, if d_label is not NULL, the label
 * int64 [h][w][d] each voxel picked.  amx_coupled_convex is seven of these. */
size_t amx_coupled_convex_step_scratch_bytes(int h, int w, int d);
int amx_coupled_convex_step(const float* d_ssd, const float* d_soft_hist, int j, int h, int w, int d, int disp_hw,
                            float* d_soft_out, long long* d_label, void* d_scratch, size_t scratch_bytes, void* stream);

/* inverse_consistency (convex_adam_utils.py:555-603): `iterations` Jacobi sweeps a' = (a - sample(b, id + a)) / 2,
 * b' = (b - sample(a, id + b)) / 2 over two fields [3][h][w][d] in normalised coordinates (channel 0 = x = last axis;
 * F.grid_sample / F.affine_grid defaults).  One launch per sweep; the inputs are not modified; the four output / input
 * buffers must be distinct.  d_scratch: amx_inverse_consistency_scratch_bytes(h, w, d). */
size_t amx_inverse_consistency_scratch_bytes(int h, int w, int d);
int amx_inverse_consistency(const float* d_field1, const float* d_field2, int h, int w, int d, int iterations, float* d_out1,
                            float* d_out2, void* d_scratch, size_t scratch_bytes, void* stream);

/* F.interpolate(x, size=(H, W, D), mode="trilinear", align_corners=False) of d_in [c][h][w][d] -> d_out [c][H][W][D], any
 * sizes, c <= 16.  Output channel k reads input channel (flip_channels ? c - 1 - k : k) multiplied by scale[k]; `scale` is
 * a HOST array of c floats (copied at the call; NULL = 1). */
int amx_resize_trilinear3d(const float* d_in, int c, int h, int w, int d, float* d_out, int H, int W, int D, const float* scale,
                           int flip_channels, void* stream);

/* run_stage1_registration (instance_optimization.py:122-222) from the pooled features d_feat_fix / d_feat_mov
 * [n_ch][h][w][d]: correlate + coupled_convex, and with ic != 0 the reverse direction, 15 consistency sweeps and the
 * upsampling, all enqueued on `stream` without host synchronisation.  ic == 0: d_disp_out [3][h][w][d] in grid units
 * (the reference does not upsample in that branch; H, W, D are ignored).  ic != 0: d_disp_out [3][H][W][D] in voxels.
 * d_scratch: amx_stage1_registration_scratch_bytes(h, w, d, disp_hw, ic). */
size_t amx_stage1_registration_scratch_bytes(int h, int w, int d, int disp_hw, int ic);
int amx_stage1_registration(const float* d_feat_fix, const float* d_feat_mov, int n_ch, int h, int w, int d, int disp_hw,
                            int grid_sp, int ic, int H, int W, int D, float* d_disp_out, void* d_scratch, size_t scratch_bytes,
                            void* stream);

/* ---- registration stage 2: the Adam instance optimisation that follows stage 1, and the warp (csrc/amx_reginstopt.hip;
 * fp32, planar [C][h][w][d], batch 1, on `stream` without host synchronisation).  Every entry validates its arguments and
 * returns an error without launching anything.  The optimisation grid needs h, w, d >= 2 (the reference divides by n - 1 and
 * takes means over n - 1 slices) and c >= 1. ---- */

/* apply_avg_pool3d(x, 3, 3) of a 3-channel field (instance_optimization.py:332-334): three zero-padded box-3 passes in ONE
 * launch, bit for bit what three amx_box_filter3d(k = 3) calls give.  Each pass is symmetric, so this is also the adjoint the
 * backward needs.  d_in, d_out [3][h][w][d], distinct buffers. */
int amx_instance_opt_smooth3(const float* d_in, float* d_out, int h, int w, int d, void* stream);

/* One iteration's forward and backward from given state (instance_optimization.py:330-382 without the step): d_weight
 * [3][h][w][d] (the Conv3d weight of create_warp, in grid cells; channel 0 moves along h), d_fix / d_mov [c][h][w][d] (the
 * pooled features) -> d_grad_weight [3][h][w][d] = d(loss + reg) / d weight with
 *   disp_sample = three box-3 passes of weight,
 *   loss = mean_voxels(mean_c((grid_sample(mov, identity + disp_sample / ((n - 1) / 2)) - fix)^2) * 12)   (bilinear, zeros, align_corners=False),
 *   reg  = lambda * diffusion_regularizer(disp_sample)                                                     (convex_adam_utils.py:81-102).
 * d_disp_sample [3][h][w][d] (nullable) receives disp_sample; d_loss2 (nullable) two floats {loss, reg}, summed in a fixed
 * order (run-to-run identical).  Three launches, four with d_loss2.  d_scratch: amx_instance_opt_scratch_bytes(c, h, w, d). */
size_t amx_instance_opt_scratch_bytes(int c, int h, int w, int d);
int amx_instance_opt_grad(const float* d_weight, const float* d_fix, const float* d_mov, int c, int h, int w, int d, float lambda,
                          float* d_grad_weight, float* d_disp_sample, float* d_loss2, void* d_scratch, size_t scratch_bytes,
                          void* stream);

/* Step t >= 1 of torch.optim.Adam(lr, betas = (0.9, 0.999), eps = 1e-8, no weight decay; instance_optimization.py:324-326, :384)
 * on n contiguous floats, in place -- the formula documented at amx_adamw_step with weight_decay = 0, with 1 - beta^t formed
 * in double on the host and passed by value (no device step counter). */
int amx_instance_opt_adam_step(float* d_weight, const float* d_grad, float* d_exp_avg, float* d_exp_avg_sq, long long n, double lr,
                               int t, void* stream);

/* The loop of run_instance_opt (instance_optimization.py:329-387): niter >= 1 iterations of Adam from d_weight_io (updated in
 * place, niter - 1 times) -> d_fitted [3][h][w][d], the disp_sample of the LAST iteration's forward.  The reference's last
 * backward and step do not reach its output and are not run; niter == 1 is gradient-free.  Four launches per iteration.
 * d_scratch: amx_instance_opt_scratch_bytes(c, h, w, d). */
int amx_instance_opt(float* d_weight_io, const float* d_fix, const float* d_mov, int c, int h, int w, int d, float lambda, double lr,
                     int niter, float* d_fitted, void* d_scratch, size_t scratch_bytes, void* stream);

/* run_instance_opt (instance_optimization.py:269-399) in one enqueue: avg_pool3d(grid_sp_adam) of both feature volumes
 * d_feat_fix / d_feat_mov [c][H][W][D], create_warp's initial weight (:225-266: trilinear resize of d_disp_hr [3][H][W][D] to the
 * grid, / grid_sp_adam), the loop above, the trilinear resize of disp_sample * grid_sp_adam back to (H, W, D) and, for
 * selected_smooth in {3, 5}, three box passes of that size (any other value: none, as the reference's `in [3, 5]`) -> d_out
 * [3][H][W][D] in voxels.  The inputs are not modified.  d_scratch: amx_run_instance_opt_scratch_bytes(same arguments). */
size_t amx_run_instance_opt_scratch_bytes(int c, int H, int W, int D, int grid_sp_adam, int selected_smooth);
int amx_run_instance_opt(const float* d_disp_hr, const float* d_feat_fix, const float* d_feat_mov, int c, int H, int W, int D,
                         int grid_sp_adam, float lambda, int niter, int selected_smooth, double lr, float* d_out, void* d_scratch,
                         size_t scratch_bytes, void* stream);

/* The driver's warp (run_convex_adam_with_network_feats.py:238-266): d_out[c] = F.grid_sample(d_vol[c], identity + (d_disp /
 * (n - 1) * 2).flip, padding zeros, align_corners=False); d_vol, d_out [c][H][W][D], d_disp [3][H][W][D] in voxels (channel 0
 * along H).  AMX_WARP_NEAREST rounds half to even, as nearbyint.  H, W, D >= 2. */
enum { AMX_WARP_BILINEAR = 0, AMX_WARP_NEAREST = 1 };
int amx_warp3d(const float* d_vol, int c, const float* d_disp, int H, int W, int D, int mode, float* d_out, void* stream);

/* ---- segmentation finetuning: what follows the UNet in anatomix/segmentation/train_segmentation.py (csrc/amx_segloss.hip;
 * fp32, planar NCDHW, on `stream` without host synchronisation or allocation; sums cross workgroups through a partial slab in
 * d_scratch added in a fixed order, so results are bit-identical from run to run).  d_in is either the UNet's features
 * x [n][feat][voxels] with the 1x1x1 head d_w [classes][feat], d_b [classes] (nullable) applied in registers (head mode,
 * 1 <= feat <= 64: segmentation_utils.py:113-115), or the logits z [n][classes][voxels] themselves (feat == 0; d_w, d_b
 * ignored).  2 <= classes <= 32.  d_labels [n][voxels] holds class indices as fp32 (truncated toward zero, as .long()), int64
 * or uint8.  Every entry validates its arguments and returns an error without launching anything. ---- */
enum { AMX_SEG_LABEL_F32 = 0, AMX_SEG_LABEL_I64 = 1, AMX_SEG_LABEL_U8 = 2 };

/* bytes of d_scratch for the forward and the backward below (0 for arguments outside the envelope) */
size_t amx_seg_loss_scratch_bytes(int n, long long voxels, int classes, int feat);

/* monai DiceCELoss(softmax=True, to_onehot_y=True) as train_segmentation.py:105-107 builds it and :144-146 calls it, and with
 * lambda_ce == 0 (the cross-entropy work is skipped) the DiceLoss of :109-111, :200.  With p = softmax(z, classes),
 * t = one_hot(labels) and, per sample b and class c, I = sum_v p t, P = sum_v p, G = sum_v t:
 *   dice = mean over (b, c in S) of 1 - (2 I + smooth_nr) / (G + P + smooth_dr),  S = all classes, without class 0 unless include_background
 *   ce   = mean over all n * voxels voxels of -log p[label]   (every class: include_background only reaches the Dice term)
 * d_loss [3] = {lambda_dice * dice + lambda_ce * ce, dice, ce}; d_stats [n][classes][3] = {I, P, G}, which the backward reads;
 * d_bad_labels [1] = the number of labels outside [0, classes): when it is not 0 the three losses are NaN (a label is only ever
 * compared with class indices, never used as an address).  Two launches. */
int amx_seg_loss_forward(const float* d_in, int feat, const float* d_w, const float* d_b, const void* d_labels, int label_dtype, int n,
                         int classes, long long voxels, int include_background, float smooth_nr, float smooth_dr, float lambda_dice,
                         float lambda_ce, float* d_loss, float* d_stats, long long* d_bad_labels, void* d_scratch,
                         size_t scratch_bytes, void* stream);

/* The adjoint of the above (what loss.backward() computes at train_segmentation.py:147 through the loss and the head), from the
 * same inputs, the forward's d_stats and the incoming gradient of the total loss d_gout [1], a DEVICE scalar (no host read).
 * Logits mode: d_dx [n][classes][voxels] = d loss / d z; d_dw, d_db, d_scratch may be NULL.  Head mode: d_dx [n][feat][voxels]
 * = W^T dz, d_dw [classes][feat] = sum_v dz x^T, d_db [classes] = sum_v dz; the logits and the softmax are recomputed from x.
 * d_dx must not alias d_in.  One launch, two in head mode. */
int amx_seg_loss_backward(const float* d_in, int feat, const float* d_w, const float* d_b, const void* d_labels, int label_dtype, int n,
                          int classes, long long voxels, int include_background, float smooth_nr, float smooth_dr, float lambda_dice,
                          float lambda_ce, const float* d_stats, const float* d_gout, float* d_dx, float* d_dw, float* d_db,
                          void* d_scratch, size_t scratch_bytes, void* stream);

/* The post-transform of train_segmentation.py:84-86 (softmax, then argmax; the softmax does not change an arg-max): d_out
 * uint8 [n][voxels] = the class of the largest logit, the lowest index on ties.  One launch. */
int amx_seg_argmax(const float* d_in, int feat, const float* d_w, const float* d_b, int n, int classes, long long voxels,
                   unsigned char* d_out, void* stream);

/* ---- registration metrics: the Dice score the reference's driver prints and the Jacobian determinant of the fitted map
 * (csrc/amx_regmetrics.hip; fp32 or integer data, planar, batch 1, on `stream` without host synchronisation or allocation;
 * bit-identical from run to run).  Every entry validates its arguments and returns an error without launching anything. ---- */

/* What sklearn.metrics.f1_score needs from the two label maps (run_convex_adam_with_network_feats.py:283-295, which copies both
 * maps to the host): d_a, d_b hold `voxels` labels each as fp32, int64 or uint8 (AMX_SEG_LABEL_*, one code per volume);
 * d_counts [bins][3] = {#(a == l), #(b == l), #(a == l and b == l)} for l in [0, bins), 1 <= bins <= 1024; d_bad [1] = the number
 * of voxels where either value is not an integer in [0, bins) (a fractional fp32 value, a negative one, NaN, one >= bins).  Such
 * a voxel is left out of all three counts, in both volumes.  An fp32 label is compared, never truncated, and no label is used as an
 * address before its range check.  The call zeroes both outputs first.  Per label the Dice (F1) score is
 * 2 counts[l][2] / (counts[l][0] + counts[l][1]).  Two launches; integer atomics only, so the counts are exact. */
int amx_label_overlap(const void* d_a, int dtype_a, const void* d_b, int dtype_b, long long voxels, int bins, long long* d_counts,
                      long long* d_bad, void* stream);

/* JacobianDet(y_pred, generate_grid((H, W, D))) (convex_adam_utils.py:226-282) for y_pred = disp.permute(1, 2, 3, 0).flip(-1):
 * d_disp [3][H][W][D] in voxels, channel a along axis a (the layout of amx_warp3d and amx_run_instance_opt), H, W, D >= 2 ->
 * d_jdet [H-1][W-1][D-1] (nullable), at (i, j, k) the determinant of the 3x3 matrix whose column a is the forward difference
 * along axis a of the map x + u (add_identity != 0: u is differenced and 1 added on the diagonal) or of u itself
 * (add_identity == 0, for a field that already holds the map); and d_stats [6] (nullable, not both) over that field =
 * {share of determinants <= 0 (folding), min, max, mean, mean of log(det) over the positive ones (NaN when there is none),
 * population standard deviation of that log (0 with fewer than two)}, accumulated in double.  d_jdet must not overlap d_disp.
 * d_scratch: amx_jacobian_det_scratch_bytes(H, W, D), only read with d_stats (0 for arguments outside the envelope).  One launch,
 * two with d_stats. */
size_t amx_jacobian_det_scratch_bytes(int H, int W, int D);
int amx_jacobian_det(const float* d_disp, int H, int W, int D, int add_identity, float* d_jdet, float* d_stats, void* d_scratch,
                     size_t scratch_bytes, void* stream);

/* ---- segmentation finetuning: the augmentation chain of get_train_transforms (segmentation_utils.py:159-216) on a batch
 * (csrc/amx_segaug.hip; fp32 NCDHW with one channel, labels fp32 or uint8 in and uint8 out, on `stream` without host
 * synchronisation, read-back or allocation).  A batch is one launch per stage with the sample on grid.y, so the number of launches
 * does not depend on n.  What differs per sample sits in a table of n amx_segaug_sample records that the caller fills on the
 * host and copies to the device once per batch: every entry takes the host copy h_table (read for validation only) and the device
 * copy d_table (read by the kernels).  A sample whose switch for a stage is off is copied through that stage bit for bit.
 * Minimum and maximum go through per-workgroup partials in d_scratch and a finalize launch; no float atomics, so a batch is
 * bit-identical from run to run.  16-byte accesses where voxels % 4 == 0 and the bases are 16-byte aligned, scalar ones
 * otherwise.  MONAI is not a dependency: its documented algorithms are restated and parity with an
 * installed MONAI is not pinned.  Every entry validates its arguments and returns an error without launching anything. ---- */
enum {
  AMX_SEGAUG_NOISE = 1,      /* RandGaussianNoise */
  AMX_SEGAUG_BIAS = 2,       /* RandBiasField(degree=3) */
  AMX_SEGAUG_GIBBS = 4,      /* RandGibbsNoise: the caller's FFTs; no kernel reads this bit */
  AMX_SEGAUG_CONTRAST = 8,   /* RandAdjustContrast */
  AMX_SEGAUG_SMOOTH = 16,    /* RandGaussianSmooth */
  AMX_SEGAUG_SHARPEN = 32,   /* RandGaussianSharpen */
  AMX_SEGAUG_AFFINE = 64,    /* RandAffine: the caller stores the identity in `affine` when it is off */
  AMX_SEGAUG_RESCALE = 128   /* ScaleIntensity */
};
enum { AMX_SEGAUG_OP_SCALE = 0, AMX_SEGAUG_OP_CONTRAST = 1 };
enum { AMX_SEGAUG_GAUSS_SMOOTH = 0, AMX_SEGAUG_GAUSS_SHARPEN = 1 };

typedef struct amx_segaug_sample {
  const float* vol;          /* the sample's resident volume [vol_dim[0]][vol_dim[1]][vol_dim[2]] (crop stage only) */
  const void* lab;           /* its label map, same shape, fp32 or uint8 (crop stage only) */
  int32_t flags;             /* AMX_SEGAUG_* switches */
  int32_t vol_dim[3];
  int32_t corner[3];         /* first voxel of the crop inside the volume */
  float noise_std;
  float bias[20];            /* c_ijk, i + j + k <= 3, (i, j, k) in lexicographic order; i runs along the first spatial axis */
  float gibbs_r;             /* radius of the k-space mask (kept here so that one copy carries every parameter) */
  float gamma;
  int32_t radius[3][3];      /* Gaussian tail per [filter: smooth, sharpen sigma1, sharpen sigma2][axis], 0 <= radius <= 4 */
  float taps[3][3][9];       /* its 2 radius + 1 taps, tap k (-radius <= k <= radius) at index k + radius */
  float sharpen_alpha;
  float affine[9];           /* A, row major: source = A (o - (size_out - 1) / 2) + (size_in - 1) / 2 */
} amx_segaug_sample;

/* sizeof(amx_segaug_sample), for a caller that lays the table out without this header */
size_t amx_segaug_sample_bytes(void);
/* bytes of d_scratch for the entries below that take it (0 for arguments outside the envelope) */
size_t amx_segaug_scratch_bytes(int n, long long voxels);

/* d_minmax [n][2] = {min, max} of each sample of d_x [n][voxels].  Two launches. */
int amx_segaug_minmax(const float* d_x, int n, long long voxels, float* d_minmax, void* d_scratch, size_t scratch_bytes, void* stream);
/* The same from the partials that amx_segaug_affine left in d_scratch for its image output (same n, voxels).  One launch. */
int amx_segaug_minmax_finalize(const void* d_scratch, size_t scratch_bytes, int n, long long voxels, float* d_minmax, void* stream);

/* One pointwise stage with the statistics d_minmax [n][2] of its own input, d_out may be d_in.  One launch.
 *   AMX_SEGAUG_OP_SCALE (switch AMX_SEGAUG_RESCALE): (x - min) / (max - min); x * 0 when min == max
 *   AMX_SEGAUG_OP_CONTRAST (switch AMX_SEGAUG_CONTRAST): ((x - min) / (range + 1e-7)) ^ gamma * range + min, range = max - min */
int amx_segaug_pointwise(const float* d_in, float* d_out, int n, long long voxels, const float* d_minmax, int op,
                         const amx_segaug_sample* h_table, const amx_segaug_sample* d_table, void* stream);

/* Crop gather, noise and bias field in one pass: d_img [n][d][h][w] = (vol[corner + o] + noise_std * d_noise[o]) * exp(f(o)) with
 * f the Legendre field over linspace(-1, 1, size) per axis of the crop, each factor under its switch (d_noise [n][d][h][w]
 * standard normal, nullable when no sample has AMX_SEGAUG_NOISE); d_lab uint8 [n][d][h][w] = the label crop.  The crop must lie
 * inside every sample's volume.  One launch. */
int amx_segaug_crop(int n, int d, int h, int w, const float* d_noise, int label_dtype, float* d_img, unsigned char* d_lab,
                    const amx_segaug_sample* h_table, const amx_segaug_sample* d_table, void* stream);

/* Separable Gaussian with the table's taps, zero padding, taps not renormalised.  AMX_SEGAUG_GAUSS_SMOOTH (switch
 * AMX_SEGAUG_SMOOTH): d_out = G_0(d_in), three launches.  AMX_SEGAUG_GAUSS_SHARPEN (switch AMX_SEGAUG_SHARPEN): b = G_1(d_in),
 * d_out = b + sharpen_alpha (b - G_2(b)), six launches.  d_tmp holds 2 n d h w floats; d_in, d_out and d_tmp must not overlap.
 * A radius above 4 (sigma > 1) in a sample whose switch is on is AMX_ERR_INVALID. */
int amx_segaug_gaussian(const float* d_in, float* d_out, float* d_tmp, int n, int d, int h, int w, int mode,
                        const amx_segaug_sample* h_table, const amx_segaug_sample* d_table, void* stream);

/* Affine resample of image and label in one kernel: d_img_in, d_lab_in [n][di][hi][wi] -> d_img_out, d_lab_out [n][d][h][w].  For
 * the output voxel o the source index is A (o - (size_out - 1) / 2) + (size_in - 1) / 2.  Image: trilinear, a corner outside the
 * input contributes 0 (grid_sample's zeros padding).  Label: the voxel at the source index rounded half to even, 0 outside.
 * A source index that is integral on all three axes copies the voxel bit for bit, so the identity at equal sizes returns both
 * inputs.  The kernel also leaves the per-workgroup minimum and maximum of d_img_out in d_scratch for
 * amx_segaug_minmax_finalize.  Inputs and outputs must not overlap.  One launch. */
int amx_segaug_affine(const float* d_img_in, const unsigned char* d_lab_in, int n, int di, int hi, int wi, float* d_img_out,
                      unsigned char* d_lab_out, int d, int h, int w, const amx_segaug_sample* h_table,
                      const amx_segaug_sample* d_table, void* d_scratch, size_t scratch_bytes, void* stream);

/* ---- contrastive pretraining: the two-view augmentation of H5SupCLDataset (pretraining/data/h5supcl_dataset.py:122-178,
 * 260-303) on one pair (csrc/amx_preaug.hip; fp32 [views][d][h][w] with w contiguous, labels uint8, on `stream` without host
 * synchronisation, read-back or allocation).  One launch per stage with the view on grid.y.  What differs per view sits in a
 * table of `views` amx_preaug_view records that the caller fills on the host and copies to the device once per pair: every entry
 * takes the host copy h_table (read for validation only) and the device copy d_table (read by the kernels).  A view whose switch
 * for a stage is off is copied through that stage bit for bit.  Nothing is accumulated across threads and there are no float
 * atomics, so a pair is bit-identical from run to run.  16-byte accesses where the sizes divide by 4 and the bases are 16-byte
 * aligned, scalar ones otherwise.  TorchIO is not a dependency: its documented algorithms are restated
 * and parity with an installed TorchIO is not pinned.  Every entry validates its arguments (axes <= 2^29, fewer than 2^31 voxels
 * per view) and returns an error without launching anything. ---- */
enum {
  AMX_PREAUG_SPATIAL = 1,    /* RandomFlip and / or RandomAffine, folded into `map` (h5supcl_dataset.py:149-178, 279-290) */
  AMX_PREAUG_BLUR = 2,       /* RandomBlur (h5supcl_dataset.py:130-132) */
  AMX_PREAUG_NOISE = 4,      /* RandomNoise (h5supcl_dataset.py:133-135) */
  AMX_PREAUG_BIAS = 8,       /* RandomBiasField (h5supcl_dataset.py:136-138) */
  AMX_PREAUG_GAMMA = 16      /* RandomGamma (h5supcl_dataset.py:139-143) */
};
enum { AMX_PREAUG_MAX_RADIUS = 8 };

typedef struct amx_preaug_view {
  int32_t flags;             /* AMX_PREAUG_* switches */
  float map[12];             /* 3 x 4, row major: source index on axis a of output voxel (z, y, x) = map[4a] z + map[4a+1] y + map[4a+2] x + map[4a+3] */
  int32_t radius[3];         /* Gaussian radius per axis (d, h, w), 0 <= radius <= 8; 0 skips the axis */
  float taps[3][17];         /* its 2 radius + 1 taps, tap k (-radius <= k <= radius) at index k + radius */
  float noise_std;
  float bias[20];            /* c_ijk of the monomials z^i y^j x^k, i + j + k <= 3, (i, j, k) in lexicographic order */
  float gamma;
} amx_preaug_view;

/* sizeof(amx_preaug_view), for a caller that lays the table out without this header */
size_t amx_preaug_view_bytes(void);

/* RandomFlip + RandomAffine of the views and their shared label map in one gather launch (h5supcl_dataset.py:279-290, where the
 * transform of view A is replayed on view B; also the rigid moves of RandomMotion, h5supcl_dataset.py:144-146, with one view and no
 * label): d_in [views][d][h][w] -> d_out, d_lab_in [d][h][w] -> d_lab_out (both null, or neither; the label follows view 0's map).
 * Image: trilinear, a corner outside the input contributes the view's pad value d_minmax[2 view] (amx_segaug_minmax's output, the
 * minimum first).  Label: the voxel at the source index rounded half to even, 0 outside.  A source index that is integral on all
 * three axes copies the voxel bit for bit, so flips and the identity are exact.  Inputs and outputs must not overlap. */
int amx_preaug_spatial(const float* d_in, const unsigned char* d_lab_in, int views, int d, int h, int w, const float* d_minmax, float* d_out,
                       unsigned char* d_lab_out, const amx_preaug_view* h_table, const amx_preaug_view* d_table, void* stream);

/* RandomBlur (h5supcl_dataset.py:130-132): the separable Gaussian of scipy.ndimage.gaussian_filter with the table's taps,
 * mode='reflect' (the reflection repeats where the radius exceeds the axis).  Two launches, both served from LDS tiles: w and h
 * fused over a plane tile into d_tmp, then a march along d through a ring of planes.  d_tmp holds views d h w floats; d_in, d_out
 * and d_tmp must not overlap.  A radius above 8 (sigma > 2) in a view whose switch is on is AMX_ERR_INVALID. */
int amx_preaug_blur(const float* d_in, float* d_out, float* d_tmp, int views, int d, int h, int w, const amx_preaug_view* h_table,
                    const amx_preaug_view* d_table, void* stream);

/* RandomNoise, RandomBiasField and RandomGamma (h5supcl_dataset.py:133-143) in one pointwise launch:
 * y = x + noise_std d_noise; y *= exp(f), f the cubic polynomial of `bias` over linspace(-1, 1, size) per axis; y = sign(y) |y|^gamma,
 * each under its switch.  d_noise [views][d][h][w] standard normal, nullable when no view has AMX_PREAUG_NOISE.  d_out may be d_in. */
int amx_preaug_intensity(const float* d_in, const float* d_noise, float* d_out, int views, int d, int h, int w, const amx_preaug_view* h_table,
                         const amx_preaug_view* d_table, void* stream);

/* ---- synthetic data generation, step 2: two views per label map (synthetic-data-generation/step2_generate_views.py with
 * datagen_utils.py:475-646) on a batch (csrc/amx_synth.hip; fp32 rows [n][d][h][w] with n = 2 batch and row = 2 sample + view,
 * labels uint8 [batch][d][h][w], on `stream` without host synchronisation, read-back or allocation).  One launch per stage with
 * the row on grid.y.  What differs per row sits in a table of n amx_synth_view records that the caller fills on the host and
 * copies to the device once per batch: every entry that takes it takes the host copy h_table (read for validation only) and the
 * device copy d_table (read by the kernels).  A row whose switch for a stage is off passes that stage bit for bit.  Minimum and
 * maximum leave per-workgroup partials in d_scratch in the layout of amx_segaug_minmax_finalize (same rows, voxels), which turns
 * them into [n][2]; sums are two-level in a fixed order; no float atomics, so a batch is bit-identical from run to run.  16-byte
 * accesses where voxels % 4 == 0 and the bases are aligned, scalar ones otherwise.  The stages the segmentation chain already has
 * (ScaleIntensity, bias field, AdjustContrast, Gaussian smooth and sharpen) are the amx_segaug_* entries.  MONAI is not a
 * dependency: KSpaceSpikeNoise and SimulateLowResolution are restated from their documented algorithms
 * and parity with an installed MONAI is not pinned.  Every entry validates its arguments and returns an error without launching
 * anything. ---- */
enum {
  AMX_SYNTH_ZERO_BACKGROUND = 1, /* sample_gmm skipped the first label: rank 0 is exactly 0 */
  AMX_SYNTH_SPIKE = 2,           /* RandKSpaceSpikeNoise */
  AMX_SYNTH_SPIKE_FIXED = 4,     /* the spike's log-magnitude is spike_intensity, not spike_factor * 2.5 * mean(log(|k| + 1e-10)) */
  AMX_SYNTH_LOWRES = 8           /* RandSimulateLowResolution */
};
enum { AMX_SYNTH_MAX_SCALES = 8 };

typedef struct amx_synth_view {
  int32_t flags;             /* AMX_SYNTH_* switches */
  int32_t nlabels;           /* number of distinct labels of the sample, 1 .. 256 */
  uint8_t rank[256];         /* label -> its position among the sample's sorted distinct labels (labels not present: anything < nlabels) */
  float mean[256];           /* per rank */
  float std[256];
  float perl_mult;           /* view = s * (1 + perl_mult * P) */
  int32_t spike_loc[3];      /* index of the spike in the SHIFTED k-space (fftshift), 0 <= loc < size */
  int32_t spike_slot;        /* row of d_k (and of d_logk_mean) that holds this row's transform */
  float spike_factor;        /* u of k_intensity = u * 2.5 * mean(log(|k| + 1e-10)) */
  float spike_intensity;     /* k_intensity itself under AMX_SYNTH_SPIKE_FIXED */
  int32_t lowres[3];         /* size of the low-resolution grid, 1 <= lowres <= size */
} amx_synth_view;

/* sizeof(amx_synth_view), for a caller that lays the table out without this header */
size_t amx_synth_view_bytes(void);
/* bytes of d_scratch for the entries below that take it, for `rows` rows (0 for arguments outside the envelope); never less than
 * amx_segaug_scratch_bytes(rows, voxels) */
size_t amx_synth_scratch_bytes(int rows, long long voxels);

/* Appearance pass 1: g = max(std[rank(label)] * noise + mean[rank(label)], 0), exactly 0 at rank 0 under
 * AMX_SYNTH_ZERO_BACKGROUND, is evaluated and not stored; d_scratch receives the min / max partials of g for the 2 batch rows.
 * d_labels [batch][voxels] is shared by a sample's two views, d_noise [2 batch][voxels] is standard normal.  A row with one label
 * and a zero background (a constant volume) is AMX_ERR_INVALID.  One launch. */
int amx_synth_gmm_minmax(const unsigned char* d_labels, const float* d_noise, int batch, long long voxels, const amx_synth_view* h_table,
                         const amx_synth_view* d_table, void* d_scratch, size_t scratch_bytes, void* stream);

/* Appearance pass 2: d_out [2 batch][d][h][w] = (g - min) / (max - min) * (1 + perl_mult * P) with {min, max} = d_gmm_minmax
 * [2 batch][2] (pass 1 finalized) and P = sum over the nscales scales of the trilinear upsample (align_corners=False, source
 * coordinate max((o + 0.5) / scale - 0.5, 0), upper neighbour clamped) of d_grids[s] [2 batch][d / scale][h / scale][w / scale];
 * d_grids and scales are HOST arrays of nscales entries.  g and P are evaluated on the fly; the coarse values a workgroup's tile
 * needs are interpolated along d and h into LDS first.  Every scale must divide d, h and w (AMX_ERR_SHAPE otherwise, as for a w
 * whose collapsed rows exceed 48 KiB of LDS).  d_scratch receives the min / max partials of d_out.  One launch. */
int amx_synth_appearance(const unsigned char* d_labels, const float* d_noise, const float* const* d_grids, const int* scales, int nscales,
                         const float* d_gmm_minmax, float* d_out, int batch, int d, int h, int w, const amx_synth_view* h_table,
                         const amx_synth_view* d_table, void* d_scratch, size_t scratch_bytes, void* stream);

/* d_mean [rows] = mean over a row of log(|k| + 1e-10), d_k [rows][voxels] complex64 (interleaved, 8-byte aligned; fftn's
 * output, shifted or not).  Per-thread double sums, a tree per workgroup, a second level over the partials.  Two launches. */
int amx_synth_logk_mean(const float* d_k, int rows, long long voxels, float* d_mean, void* d_scratch, size_t scratch_bytes, void* stream);

/* KSpaceSpikeNoise without the inverse transform, in place on the rows with AMX_SYNTH_SPIKE (the others are not touched):
 * setting log|k| at spike_loc of the shifted k-space to k_intensity with the phase kept adds one plane wave,
 *   x(r) += Re(delta / N * exp(2 pi i sum_a f_a r_a / n_a)),  f_a = (loc_a - n_a / 2) mod n_a,  delta = exp(k_intensity) k[f] / |k[f]| - k[f]
 * (phase 0 where k[f] = 0).  d_k [k_rows][d][h][w] complex64 is the UNSHIFTED fftn of the rows, row spike_slot for each of
 * them; d_logk_mean [k_rows] is amx_synth_logk_mean's output (nullable when every spike is AMX_SYNTH_SPIKE_FIXED).  The phase
 * is reduced modulo n_a in integers before the sine and cosine.  One launch. */
int amx_synth_spike(float* d_x, const float* d_k, int k_rows, const float* d_logk_mean, int n, int d, int h, int w, const amx_synth_view* h_table,
                    const amx_synth_view* d_table, void* stream);

/* SimulateLowResolution(downsample_mode="nearest-exact", upsample_mode="trilinear", align_corners=False) as one gather: each
 * output voxel blends the 8 low-resolution neighbours of its source coordinate, each of them read at its nearest-exact source
 * voxel of d_in; float32 index arithmetic as torch's.  Rows without AMX_SYNTH_LOWRES are copied.  d_in and d_out must not
 * overlap.  One launch. */
int amx_synth_lowres(const float* d_in, float* d_out, int n, int d, int h, int w, const amx_synth_view* h_table, const amx_synth_view* d_table,
                     void* stream);

/* The tail.  amx_synth_clip_minmax: the min / max partials of max(x, 0) (ThresholdIntensity(above=True, threshold=0) folded into
 * the statistics pass) into d_scratch.  amx_synth_finish: ScaleIntensity of max(x, 0) with d_minmax [n][2] ((c - min) / (max - min);
 * c * 0 when min == max) as float32, or with out_u8 != 0 as uint8 trunc(255 * y); d_out may be d_in for float32.  One launch each. */
int amx_synth_clip_minmax(const float* d_x, int n, long long voxels, void* d_scratch, size_t scratch_bytes, void* stream);
int amx_synth_finish(const float* d_in, void* d_out, int n, long long voxels, const float* d_minmax, int out_u8, void* stream);

/* ---- synthetic data generation, step 1: label ensembles (synthetic-data-generation/step1_generate_labels.py with
 * datagen_utils.py:26-447) on a batch (csrc/amx_labels.hip).  All volumes are uint8 [batch][d][h][w], on
 * `stream` without host synchronisation, read-back or allocation, one launch per stage with the ensemble on a grid axis.  What
 * differs per ensemble sits in a table of `batch` amx_labels_ensemble records, and what differs per template in a table of
 * amx_labels_template records; both are filled on the host and copied to the device once per batch, and every entry takes the
 * host copy (read for validation only) and the device copy (read by the kernels).  An ensemble whose switch for a stage is off
 * passes that launch bit for bit.  Integer arithmetic and fixed-order float arithmetic only: two runs agree bit for bit.  Every
 * entry validates its arguments and returns an error without launching anything. ---- */
enum {
  AMX_LABELS_MASK = 1,     /* the deformed-sphere foreground mask (step1_generate_labels.py:101-116) */
  AMX_LABELS_ENVELOPE = 2  /* the envelope around it (step1_generate_labels.py:119-138); needs AMX_LABELS_MASK */
};
enum { AMX_LABELS_MAX_TEMPLATES = 64 };

typedef struct amx_labels_template {
  int64_t offset;   /* of the cropped template [c0][c1][c2] in the byte buffer */
  int32_t crop[3];  /* c: shape of the non-zero bounding box */
  int32_t before[3];/* p: zero voxels in front of it, pad / 2 + (pad & 1) with pad = padded - crop */
  int32_t padded[3];/* P = max(size, c): the wrap period */
  int32_t reserved;
  double affine[12];/* rows (M_a0, M_a1, M_a2, t_a) of the output -> source map */
} amx_labels_template;

typedef struct amx_labels_ensemble {
  int32_t flags;       /* AMX_LABELS_* switches */
  int32_t first, count;/* its templates: records first .. first + count - 1, 1 <= count <= AMX_LABELS_MAX_TEMPLATES */
  int32_t radius;      /* of the sphere, >= 0 */
  int32_t shift[3];    /* of its centre from size / 2, per axis (d, h, w) */
  int32_t ball;        /* radius of the envelope's ball: 2, 3 or 4 */
} amx_labels_ensemble;

/* sizeof the two records, for a caller that lays the tables out without this header */
size_t amx_labels_template_bytes(void);
size_t amx_labels_ensemble_bytes(void);
/* bytes of d_scratch of amx_labels_apply_mask (0 for arguments outside the envelope) */
size_t amx_labels_scratch_bytes(int batch, long long voxels);

/* Compose (step1_generate_labels.py:69-95, datagen_utils.py:71-194): d_out [batch][d][h][w] is, per voxel o, the largest k whose
 * template has a non-zero sample there, else 0 -- the reference's in-order `label_ensemble[roi > 0] = k`.  Template k's sample is
 * scipy's affine_transform(order=0, mode='grid-wrap') of the cropped and padded template without materialising it:
 * x_a = t_a + o_0 M_a0 + o_1 M_a1 + o_2 M_a2 in float64 in that order without contraction, i_a = floor(x_a + 0.5) mod P_a, and the
 * value is the cropped template at i - p, 0 outside it.  d_templates: template_bytes bytes, any alignment.  One launch. */
int amx_labels_compose(const unsigned char* d_templates, size_t template_bytes, const amx_labels_template* h_templates,
                       const amx_labels_template* d_templates_table, int ntemplates, const amx_labels_ensemble* h_table,
                       const amx_labels_ensemble* d_table, unsigned char* d_out, int batch, int d, int h, int w, void* stream);

/* The exact 3 x 3 x 3 median of uint8 with border replication (step1_generate_labels.py:98, 111: skimage.filters.median's default
 * footprint and mode='nearest'): element 13 of the 27 sorted neighbours, for a 0 / 1 mask "at least 14 of 27".  Ensembles whose
 * flags lack one of the bits of `require` are copied.  d_in and d_out must not overlap.  One launch. */
int amx_labels_median3(const unsigned char* d_in, unsigned char* d_out, int batch, int d, int h, int w, int require,
                       const amx_labels_ensemble* h_table, const amx_labels_ensemble* d_table, void* stream);

/* The deformed-sphere foreground mask (datagen_utils.py:371-447, negated as at step1_generate_labels.py:107-110) of the ensembles
 * with AMX_LABELS_MASK as one fused kernel; the others' volumes are not touched.  d_grids: HOST array of 3 device pointers, the
 * coarse Gaussian grids [batch][3][size / s]^3 float32 of the scales s = size / 16, size / 8, size / 4, already multiplied by
 * their std.  Per voxel and component c (0 indexes w, 1 h, 2 d), float32 in torch's order of operations (products and sums of the
 * blends rounded one by one; the blend weight may differ from torch's in the last bit): the displacement is the sum over the scales of
 * the trilinear upsample (align_corners=False), g = base(o) + 2 disp / (size - 1), x = ((g + 1) size - 1) / 2, reflected about
 * [-0.5, size - 0.5], clipped to [0, size - 1] and rounded half to even to q; the mask is 1 where
 * |q - (size / 2 + shift)|^2 <= radius^2 in integers.  Cubes with size % 16 == 0, 16 <= size <= 256.  One launch. */
int amx_labels_sphere_mask(const float* const* d_grids, unsigned char* d_mask, int batch, int size, const amx_labels_ensemble* h_table,
                           const amx_labels_ensemble* d_table, void* stream);

/* step1_generate_labels.py:115-116 in place: label = mask ? label + 1 : 0 for the ensembles with AMX_LABELS_MASK, and
 * d_max [batch] int32 = the maximum label of every ensemble afterwards (per-workgroup partials in d_scratch, then a finalize
 * launch).  Two launches. */
int amx_labels_apply_mask(unsigned char* d_labels, const unsigned char* d_mask, int* d_max, int batch, long long voxels,
                          const amx_labels_ensemble* h_table, const amx_labels_ensemble* d_table, void* d_scratch, size_t scratch_bytes,
                          void* stream);

/* step1_generate_labels.py:123-138 in place for the ensembles with AMX_LABELS_ENVELOPE: label = 1 + d_max[ensemble] where
 * dilate(mask, ball) & ~erode(mask, ball), ball = {x^2 + y^2 + z^2 <= ball^2}, the border scipy's `reflect` (the edge voxel
 * repeated; skimage's default for both operators), erosion evaluated as ~dilate(~mask).  Rows packed as bits in LDS; the ball is
 * a union of x-runs.  Every axis must be at least 9.  One launch. */
int amx_labels_envelope(unsigned char* d_labels, const unsigned char* d_mask, const int* d_max, int batch, int d, int h, int w,
                        const amx_labels_ensemble* h_table, const amx_labels_ensemble* d_table, void* stream);

/* ---- synthetic data generation, step 0: the merge of a TotalSegmentator segmentation folder
 * (synthetic-data-generation/step0_preprocess_totalsegmentator.py:57-76: `segdata.sum() == 0`, `rib_labels += segdata`,
 * `vert_labels += segdata`) for a batch of its mask files in one pass and one launch (csrc/amx_labels.hip).
 * d_masks: n rows of uint8, `stride` bytes apart (stride % 16 == 0, stride >= voxels, 16-byte aligned base), the first `voxels`
 * bytes of a row being the file.  h_group: HOST array of n entries, 0 = neither, 1 = rib, 2 = vertebra.  d_merged: [2][stride]
 * uint8, row 0 the ribs, row 1 the vertebrae; with accumulate == 0 it is written (all zero for a group without files), otherwise
 * the batch is added to what it holds.  d_sums: n + 2 uint64, written: [i] the sum of the voxels of file i (0 = the file is blank),
 * [n] and [n + 1] the sums of the two merged rows as they stand after the call.  d_overflow: 2 int32, zeroed when accumulate == 0,
 * then set to 1 for a group one of whose merged voxels passed 255 (the stored voxel is 255 then); with accumulate != 0 a flag stays
 * set.  Integer arithmetic only: the result does not depend on the order of anything.  1 <= n <= AMX_LABELS_MAX_MERGE,
 * 1 <= voxels < 2^31. */
enum { AMX_LABELS_MAX_MERGE = 256 };
int amx_labels_merge_masks(const unsigned char* d_masks, int n, long long voxels, long long stride, const int* h_group,
                           unsigned char* d_merged, unsigned long long* d_sums, int* d_overflow, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ANATOMIX_AMD_H */
