// anatomix_amd -- the 3D ViT variant `anatomix-dev-vit` (PrimusV2-S) as ONE C-ABI forward: conv tokenizer -> EVA blocks ->
// patch decoder -> ChannelDemean, every kernel from this library (amx_tokenizer.hip, amx_gemm.hip, amx_attention.hip).
// Reference surface: anatomix/model/vit3d/architectures.py:231-260 (PrimusV2), :89-165 (_PrimusExtensions), deep_tokenizer.py:12-68,
// registry entry load_from_hf.py:25-35; the upstream blocks (dynamic-network-architectures / timm, absent from this image) are
// restated in oracle/vit_ref.py -- PARITY WITH THE UPSTREAM PACKAGE IS UNPINNED, see there.
//
// Precision plan (rel-L2 against the fp32 restatement, measured per choice in DESIGN.md section 8):
//   tokenizer      fp32 raw conv outputs, hi + lo f16 activations and weights, 3 MFMAs per product (ten InstanceNorms in a row);
//   EVA blocks     fp32 residual stream, f16 operands (LayerNorm outputs, weights, q / k / v / p), fp32 accumulate;
//   decoder        hi + lo operands (cfg.decoder_split), fp32 raw outputs, LayerNorm + GELU in fp32.
#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "amx_gemm.h"
#include "amx_launch.h"

namespace {

using amx::fail;

inline int up(int v, int m) { return (v + m - 1) / m * m; }

struct Packed {            // one packed matrix (hi [+ lo]) in the parameter arena
  char* hi = nullptr;
  char* lo = nullptr;
  int ntiles = 0, KS = 0;
};

struct Arena {
  char* base = nullptr;
  size_t off = 0;
  template <typename T = char>
  T* take(size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? (T*)(base + off) : nullptr;
    off += bytes;
    return p;
  }
};

struct Block {
  float *n1w, *n1b, *qkb, *vb, *qnw, *qnb, *knw, *knb, *anw, *anb, *projb, *g1, *n2w, *n2b, *fc1b, *mnw, *mnb, *fc2b, *g2;
  Packed qk, v, proj, fc1, fc2;       // q | k and v projections with every head padded to 80 features (5 tiles)
};
struct Stage {
  Packed c1, c2, sk;
  float *c1b, *n1w, *n1b, *c2b, *n2w, *n2b, *snw, *snb;
  int cin, cout;
};
struct DecStage {
  Packed w;
  float *bias, *lnw, *lnb;
  const float* w_raw;       // fp32 copy of the LAST stage's weight (ChannelDemean through linearity)
  int cin, cout, cp;
};

}  // namespace

struct amx_vit {
  amx_vit_cfg cfg;
  int E, Ep, hd, V, T, hidden;                 // embed dim, padded to 32, head dim, patch tokens, tokens per sample
  std::vector<std::string> names;              // parameter slots in load order
  bool loaded = false;
  char* params = nullptr;                      // one device allocation for everything packed
  size_t params_bytes = 0;
  // tokenizer
  Packed stem_w;
  float *stem_b, *stem_nw, *stem_nb;
  Stage st[3];
  Packed tokproj;
  float *tokproj_b, *pos, *regs, *rope;
  std::vector<Block> blk;
  float *fnw, *fnb;
  DecStage dec[3];
  amx::SwMapCache sw_map;      // amx_vit_sliding_window: the window weights of the handle's roi
};

namespace {

const int kStageC[4] = {32, 32, 64, 128};

void build_names(amx_vit* h) {
  auto& n = h->names;
  const amx_vit_cfg& c = h->cfg;
  n = {"down_projection.stem.conv.weight", "down_projection.stem.conv.bias", "down_projection.stem.norm.weight", "down_projection.stem.norm.bias"};
  for (int k = 0; k < 3; ++k) {
    const std::string p = "down_projection.stages." + std::to_string(k);
    for (const char* s : {".conv1.weight", ".conv1.bias", ".norm1.weight", ".norm1.bias", ".conv2.weight", ".conv2.bias", ".norm2.weight", ".norm2.bias",
                          ".skip.weight", ".skip_norm.weight", ".skip_norm.bias"})
      n.push_back(p + s);
  }
  n.push_back("down_projection.proj.weight");
  n.push_back("down_projection.proj.bias");
  if (c.num_register_tokens > 0) n.push_back("register_tokens");
  n.push_back("eva.pos_embed");
  for (int b = 0; b < c.depth; ++b) {
    const std::string p = "eva.blocks." + std::to_string(b);
    for (const char* s : {".norm1.weight", ".norm1.bias", ".attn.q_proj.weight", ".attn.q_proj.bias", ".attn.k_proj.weight", ".attn.v_proj.weight",
                          ".attn.v_proj.bias", ".attn.proj.weight", ".attn.proj.bias"})
      n.push_back(p + s);
    if (c.qk_norm)
      for (const char* s : {".attn.q_norm.weight", ".attn.q_norm.bias", ".attn.k_norm.weight", ".attn.k_norm.bias"}) n.push_back(p + s);
    if (c.scale_attn_inner)
      for (const char* s : {".attn.norm.weight", ".attn.norm.bias"}) n.push_back(p + s);
    if (c.layer_scale) n.push_back(p + ".gamma_1");
    for (const char* s : {".norm2.weight", ".norm2.bias", ".mlp.fc1_g.weight", ".mlp.fc1_g.bias", ".mlp.fc1_x.weight", ".mlp.fc1_x.bias", ".mlp.norm.weight",
                          ".mlp.norm.bias", ".mlp.fc2.weight", ".mlp.fc2.bias"})
      n.push_back(p + s);
    if (c.layer_scale) n.push_back(p + ".gamma_2");
  }
  n.push_back("eva.norm.weight");
  n.push_back("eva.norm.bias");
  for (int k = 0; k < 3; ++k) {
    const std::string p = "up_projection.decode." + std::to_string(k);
    if (k < 2) {
      for (const char* s : {".0.weight", ".0.bias", ".1.weight", ".1.bias"}) n.push_back(p + s);
    } else {
      n.push_back(p + ".weight");
      n.push_back(p + ".bias");
    }
  }
}

Packed take_packed(Arena& a, int ntiles, int KS, bool split) {
  Packed p;
  p.ntiles = ntiles;
  p.KS = KS;
  p.hi = a.take((size_t)ntiles * KS * 1024);
  if (split) p.lo = a.take((size_t)ntiles * KS * 1024);
  return p;
}

// Lays out the parameter arena (dry run with base == null gives the size).
void layout_params(amx_vit* h, Arena& a) {
  const amx_vit_cfg& c = h->cfg;
  const int E = h->E, hid = h->hidden;
  auto f = [&](int n) { return a.take<float>((size_t)n * sizeof(float)); };
  h->stem_w = take_packed(a, 2, 1, true);
  h->stem_b = f(32); h->stem_nw = f(32); h->stem_nb = f(32);
  for (int k = 0; k < 3; ++k) {
    Stage& s = h->st[k];
    s.cin = kStageC[k]; s.cout = kStageC[k + 1];
    s.c1 = take_packed(a, s.cout / 16, 27 * s.cin / 32, true);
    s.c2 = take_packed(a, s.cout / 16, 27 * s.cout / 32, true);
    s.sk = take_packed(a, s.cout / 16, s.cin / 32, true);
    s.c1b = f(s.cout); s.n1w = f(s.cout); s.n1b = f(s.cout); s.c2b = f(s.cout); s.n2w = f(s.cout); s.n2b = f(s.cout); s.snw = f(s.cout); s.snb = f(s.cout);
  }
  h->tokproj = take_packed(a, up(E, 16) / 16, kStageC[3] / 32, true);
  h->tokproj_b = f(up(E, 16));
  h->pos = f(h->V * E);
  h->regs = f(std::max(1, c.num_register_tokens) * E);
  h->rope = f(h->V * 2 * h->hd);
  h->blk.resize(c.depth);
  const int KSe = h->Ep / 32, KSh = up(hid, 32) / 32;
  for (auto& b : h->blk) {
    b.qk = take_packed(a, 2 * c.heads * 5, KSe, false);
    b.v = take_packed(a, c.heads * 5, KSe, false);
    b.proj = take_packed(a, up(E, 16) / 16, KSe, false);
    b.fc1 = take_packed(a, 2 * up(hid, 16) / 16, KSe, false);      // hidden rounded up to whole (gate, value) tile pairs, zero weights behind it
    b.fc2 = take_packed(a, up(E, 16) / 16, KSh, false);
    b.n1w = f(E); b.n1b = f(E); b.qkb = f(2 * c.heads * 80); b.vb = f(c.heads * 80); b.qnw = f(80); b.qnb = f(80); b.knw = f(80); b.knb = f(80);
    b.anw = f(E); b.anb = f(E); b.projb = f(up(E, 16)); b.g1 = f(up(E, 16)); b.n2w = f(E); b.n2b = f(E); b.fc1b = f(2 * up(hid, 16));
    b.mnw = f(hid); b.mnb = f(hid); b.fc2b = f(up(E, 16)); b.g2 = f(up(E, 16));
  }
  h->fnw = f(E); h->fnb = f(E);
  const int dc[4] = {E, c.dec1, c.dec2, c.num_classes};
  for (int k = 0; k < 3; ++k) {
    DecStage& d = h->dec[k];
    d.cin = dc[k]; d.cout = dc[k + 1]; d.cp = up(d.cout, 16);
    d.w = take_packed(a, 8 * d.cp / 16, up(d.cin, 32) / 32, c.decoder_split != 0);
    d.bias = f(d.cp);
    d.lnw = f(d.cout); d.lnb = f(d.cout);
    d.w_raw = k == 2 ? f(d.cin * d.cout * 8) : nullptr;
  }
}

}  // namespace

extern "C" {

int amx_vit_create(amx_vit_t** out, const amx_vit_cfg* cfg) {
  if (!out || !cfg) return fail(AMX_ERR_INVALID, "null argument");
  *out = nullptr;
  const amx_vit_cfg& c = *cfg;
  if (c.input_channels != 1) return fail(AMX_ERR_INVALID, "vit: input_channels must be 1 (got %d)", c.input_channels);
  if (c.embed_dim < 32 || c.embed_dim % 4 || c.heads < 1 || c.embed_dim % c.heads) return fail(AMX_ERR_INVALID, "vit: embed_dim %d / heads %d", c.embed_dim, c.heads);
  const int hd = c.embed_dim / c.heads;
  if ((hd & 1) || hd > 80) return fail(AMX_ERR_INVALID, "vit: head_dim must be even and <= 80 (got %d)", hd);
  if (c.depth < 1 || c.num_register_tokens < 0) return fail(AMX_ERR_INVALID, "vit: depth / register tokens");
  if (c.grid_d < 2 || c.grid_h < 2 || c.grid_w < 2 || (c.grid_w % 2) || ((long long)c.grid_d * c.grid_h * c.grid_w) % 64 || (c.grid_w * 8) % 16)
    return fail(AMX_ERR_SHAPE, "vit: token grid %dx%dx%d (even width, a multiple of 64 tokens)", c.grid_d, c.grid_h, c.grid_w);
  if (c.hidden < 16 || c.hidden > 3072 || ((c.hidden % 4) && c.hidden > 1088))
    return fail(AMX_ERR_INVALID, "vit: SwiGLU hidden width %d must be 16 .. 3072 (a multiple of 4 above 1088)", c.hidden);
  if (c.embed_dim > 1280) return fail(AMX_ERR_INVALID, "vit: embed_dim <= 1280");
  if (c.dec1 % 4 || c.dec2 % 4 || c.num_classes % 4 || c.dec1 < 4 || c.dec2 < 4 || c.num_classes < 4 || c.dec1 > 1024 || c.dec2 > 256 || c.num_classes > 128)
    return fail(AMX_ERR_INVALID, "vit: decoder widths %d / %d / %d must be multiples of 4 (<= 1024 / 256, classes <= 128)", c.dec1, c.dec2, c.num_classes);
  if (c.out_norm != 0 && c.out_norm != 1) return fail(AMX_ERR_INVALID, "vit: out_norm 0 (none) or 1 (demean)");
  amx_vit* h = new amx_vit();
  h->cfg = c;
  h->E = c.embed_dim; h->Ep = up(c.embed_dim, 32); h->hd = hd; h->hidden = c.hidden;
  h->V = c.grid_d * c.grid_h * c.grid_w;
  h->T = h->V + c.num_register_tokens;
  build_names(h);
  Arena dry;
  layout_params(h, dry);
  h->params_bytes = dry.off + 256;
  hipError_t e = hipMalloc((void**)&h->params, h->params_bytes);
  if (e != hipSuccess) { delete h; return fail(AMX_ERR_HIP, "hipMalloc(%zu): %s", dry.off, hipGetErrorString(e)); }
  Arena real;
  real.base = h->params;
  layout_params(h, real);
  *out = h;
  return AMX_OK;
}

void amx_vit_destroy(amx_vit_t* h) {
  if (!h) return;
  if (h->params) (void)hipFree(h->params);
  h->sw_map.release();
  delete h;
}

int amx_vit_num_params(const amx_vit_t* h) { return h ? (int)h->names.size() : 0; }
const char* amx_vit_param_name(const amx_vit_t* h, int idx) { return h && idx >= 0 && idx < (int)h->names.size() ? h->names[idx].c_str() : nullptr; }

int amx_vit_load(amx_vit_t* h, const float* const* d_params, int count, const float* d_rope, void* stream) {
  if (!h || !d_params || !d_rope) return fail(AMX_ERR_INVALID, "null argument");
  if (count != (int)h->names.size()) return fail(AMX_ERR_INVALID, "vit: expected %d parameter tensors, got %d", (int)h->names.size(), count);
  for (int i = 0; i < count; ++i)
    if (!d_params[i]) return fail(AMX_ERR_INVALID, "vit: parameter %s is null", h->names[i].c_str());
  hipStream_t st = (hipStream_t)stream;
  const amx_vit_cfg& c = h->cfg;
  const int E = h->E, hid = h->hidden;
  int i = 0;
  auto next = [&]() { return d_params[i++]; };
  auto vec = [&](float* dst, const float* src, int n, int npad = 0) -> hipError_t {
    hipError_t e = amx::launch_vec_place(dst, src, n, 0.f, st);
    if (e == hipSuccess && npad > n) e = amx::launch_vec_place(dst + n, nullptr, npad - n, 0.f, st);
    return e;
  };
  AMX_HIP(hipMemsetAsync(h->params, 0, h->params_bytes, st));
  AMX_HIP(amx::launch_pack_tokstem(next(), h->stem_w.hi, h->stem_w.lo, st));
  AMX_HIP(vec(h->stem_b, next(), 32));
  AMX_HIP(vec(h->stem_nw, next(), 32));
  AMX_HIP(vec(h->stem_nb, next(), 32));
  for (int k = 0; k < 3; ++k) {
    Stage& s = h->st[k];
    AMX_HIP(amx::launch_pack_tokconv(next(), s.cout, s.cin, 27, s.c1.hi, s.c1.lo, st));
    AMX_HIP(vec(s.c1b, next(), s.cout));
    AMX_HIP(vec(s.n1w, next(), s.cout));
    AMX_HIP(vec(s.n1b, next(), s.cout));
    AMX_HIP(amx::launch_pack_tokconv(next(), s.cout, s.cout, 27, s.c2.hi, s.c2.lo, st));
    AMX_HIP(vec(s.c2b, next(), s.cout));
    AMX_HIP(vec(s.n2w, next(), s.cout));
    AMX_HIP(vec(s.n2b, next(), s.cout));
    AMX_HIP(amx::launch_pack_tokconv(next(), s.cout, s.cin, 1, s.sk.hi, s.sk.lo, st));
    AMX_HIP(vec(s.snw, next(), s.cout));
    AMX_HIP(vec(s.snb, next(), s.cout));
  }
  AMX_HIP(amx::launch_pack_gemm(next(), nullptr, nullptr, E, 0, 0, kStageC[3], 0, 0, 0, h->tokproj.ntiles, h->tokproj.KS, h->tokproj.hi, h->tokproj.lo, st));
  AMX_HIP(vec(h->tokproj_b, next(), E, up(E, 16)));
  if (c.num_register_tokens > 0) AMX_HIP(vec(h->regs, next(), c.num_register_tokens * E));
  AMX_HIP(vec(h->pos, next(), h->V * E));
  AMX_HIP(amx::launch_rope_pairs(h->rope, d_rope, h->V, h->hd, st));
  for (auto& b : h->blk) {
    AMX_HIP(vec(b.n1w, next(), E));
    AMX_HIP(vec(b.n1b, next(), E));
    const float *qw = next(), *qb = next(), *kw = next(), *vw = next(), *vb = next();
    AMX_HIP(amx::launch_pack_gemm(qw, kw, nullptr, E, 0, 0, E, 4, 80, h->hd, b.qk.ntiles, b.qk.KS, b.qk.hi, nullptr, st));
    AMX_HIP(amx::launch_pack_gemm(vw, nullptr, nullptr, E, 0, 0, E, 4, 80, h->hd, b.v.ntiles, b.v.KS, b.v.hi, nullptr, st));
    AMX_HIP(amx::launch_headpad_vec(b.qkb, qb, c.heads, h->hd, 80, st));
    AMX_HIP(amx::launch_headpad_vec(b.qkb + c.heads * 80, nullptr, c.heads, h->hd, 80, st));     // EVA: the key projection has no bias
    AMX_HIP(amx::launch_headpad_vec(b.vb, vb, c.heads, h->hd, 80, st));
    AMX_HIP(amx::launch_pack_gemm(next(), nullptr, nullptr, E, 0, 0, E, 0, 0, 0, b.proj.ntiles, b.proj.KS, b.proj.hi, nullptr, st));
    AMX_HIP(vec(b.projb, next(), E, up(E, 16)));
    if (c.qk_norm) {
      AMX_HIP(vec(b.qnw, next(), h->hd, 80));
      AMX_HIP(vec(b.qnb, next(), h->hd, 80));
      AMX_HIP(vec(b.knw, next(), h->hd, 80));
      AMX_HIP(vec(b.knb, next(), h->hd, 80));
    }
    if (c.scale_attn_inner) {
      AMX_HIP(vec(b.anw, next(), E));
      AMX_HIP(vec(b.anb, next(), E));
    }
    if (c.layer_scale) AMX_HIP(vec(b.g1, next(), E, up(E, 16)));
    else AMX_HIP(amx::launch_vec_place(b.g1, nullptr, up(E, 16), 1.f, st));
    AMX_HIP(vec(b.n2w, next(), E));
    AMX_HIP(vec(b.n2b, next(), E));
    const float *gw = next(), *gb = next(), *xw = next(), *xb = next();
    AMX_HIP(amx::launch_pack_gemm(gw, xw, nullptr, hid, hid, 0, E, 1, 0, 0, b.fc1.ntiles, b.fc1.KS, b.fc1.hi, nullptr, st));
    AMX_HIP(amx::launch_swiglu_bias(b.fc1b, gb, xb, hid, st));
    AMX_HIP(vec(b.mnw, next(), hid));
    AMX_HIP(vec(b.mnb, next(), hid));
    AMX_HIP(amx::launch_pack_gemm(next(), nullptr, nullptr, E, 0, 0, hid, 0, 0, 0, b.fc2.ntiles, b.fc2.KS, b.fc2.hi, nullptr, st));
    AMX_HIP(vec(b.fc2b, next(), E, up(E, 16)));
    if (c.layer_scale) AMX_HIP(vec(b.g2, next(), E, up(E, 16)));
    else AMX_HIP(amx::launch_vec_place(b.g2, nullptr, up(E, 16), 1.f, st));
  }
  AMX_HIP(vec(h->fnw, next(), E));
  AMX_HIP(vec(h->fnb, next(), E));
  for (int k = 0; k < 3; ++k) {
    DecStage& d = h->dec[k];
    const float* w = next();
    AMX_HIP(amx::launch_pack_gemm(w, nullptr, nullptr, 0, 0, 0, d.cin, k == 2 ? 3 : 2, d.cp, d.cout, d.w.ntiles, d.w.KS, d.w.hi, d.w.lo, st));
    if (d.w_raw) AMX_HIP(vec((float*)d.w_raw, w, d.cin * d.cout * 8));
    AMX_HIP(vec(d.bias, next(), d.cout, d.cp));
    if (k < 2) {
      AMX_HIP(vec(d.lnw, next(), d.cout));
      AMX_HIP(vec(d.lnb, next(), d.cout));
    }
  }
  if (i != count) return fail(AMX_ERR_INVALID, "vit: internal parameter count mismatch (%d of %d consumed)", i, count);
  h->loaded = true;
  return AMX_OK;
}

}  // extern "C"

namespace {

// Workspace plan of one forward at batch n.  Regions: the token stream (lives across phases) + max(tokenizer, blocks, decoder).
struct Plan {
  // common
  float* tok;
  // tokenizer
  float *stats, *sc[4], *sh[4];            // statistic slots; (scale, shift) sets: 0 stem / conv1, 1 conv2, 2 skip
  char *h_hi[4], *h_lo[4], *p_hi[3], *p_lo[3];
  float *raw1, *raw2, *raws;
  char *a1_hi, *a1_lo;
  // blocks
  char *A1, *A2, *Hd, *att;
  float *AO;
  // decoder
  char *Ad_hi[3], *Ad_lo[3];
  float *rawd[3], *colsum, *mean;
  size_t total;
};

constexpr int kColChunks = 128;

Plan make_plan(const amx_vit* h, int n, char* base) {
  Plan P{};
  const amx_vit_cfg& c = h->cfg;
  const int E = h->E, Ep = h->Ep, T = h->T, V = h->V, hid = h->hidden;
  const long long M = (long long)n * T;
  Arena a;
  a.base = base;
  P.tok = a.take<float>((size_t)M * E * 4);
  const size_t common = a.off;
  // ---- tokenizer
  const long long v0 = (long long)V * 512;                 // voxels per sample at full resolution (8^3 per token)
  P.stats = a.take<float>((size_t)n * (size_t)(v0 / 256 + 64) * 128 * 2 * 4);   // upper bound: <= v0 / 256 slots per sample (32 voxels per wave at 1/8 of the input), <= 128 channels
  for (int k = 0; k < 3; ++k) { P.sc[k] = a.take<float>((size_t)n * 128 * 4); P.sh[k] = a.take<float>((size_t)n * 128 * 4); }
  long long vk = v0;
  for (int k = 0; k < 4; ++k) {
    P.h_hi[k] = a.take((size_t)n * vk * kStageC[k] * 2);
    P.h_lo[k] = a.take((size_t)n * vk * kStageC[k] * 2);
    if (k < 3) {
      P.p_hi[k] = a.take((size_t)n * (vk / 8) * kStageC[k] * 2);
      P.p_lo[k] = a.take((size_t)n * (vk / 8) * kStageC[k] * 2);
    }
    vk /= 8;
  }
  const size_t rawb = (size_t)n * (v0 / 8) * 32 * 4;      // the largest raw tensor: stage 0 output (64^3 x 32); later stages are half that
  P.raw1 = a.take<float>(rawb);
  P.raw2 = a.take<float>(rawb);
  P.raws = a.take<float>(rawb);
  P.a1_hi = a.take(rawb / 2);
  P.a1_lo = a.take(rawb / 2);
  const size_t tok_end = a.off;
  // ---- blocks (alias the tokenizer region)
  a.off = common;
  const long long Mp = (M + 255) / 256 * 256;
  P.A1 = a.take((size_t)Mp * Ep * 2);
  P.A2 = a.take((size_t)Mp * up(hid, 32) * 2);
  P.Hd = a.take((size_t)Mp * up(hid, 16) * 2);
  P.AO = a.take<float>((size_t)M * E * 4);
  P.att = a.take(amx::attention_scratch_bytes(n, c.heads, T));
  const size_t blk_end = a.off;
  // ---- decoder (aliases both)
  a.off = common;
  long long rows = (long long)n * V;
  const int dk[3] = {Ep, up(c.dec1, 32), up(c.dec2, 32)};
  for (int k = 0; k < 3; ++k) {
    P.Ad_hi[k] = a.take((size_t)rows * dk[k] * 2);
    P.Ad_lo[k] = c.decoder_split ? a.take((size_t)rows * dk[k] * 2) : nullptr;
    rows *= 8;
    P.rawd[k] = k < 2 ? a.take<float>((size_t)rows * h->dec[k].cout * 4) : nullptr;     // the last stage writes the planar output itself
  }
  P.colsum = a.take<float>((size_t)n * kColChunks * 256 * 4);
  P.mean = a.take<float>((size_t)n * 128 * 4);
  const size_t dec_end = a.off;
  P.total = std::max(tok_end, std::max(blk_end, dec_end)) + 256;
  return P;
}

// Where the last decoder product of a forward leaves its result: the planar tensor d_y [n][C][roi] (amx_vit_forward), or -- `acc`
// set -- sample i blended into the sliding-window accumulator at corner[i] (amx_vit_forward_windows; no [n][C][roi] tensor exists).
struct VitOut {
  float* y = nullptr;
  float* acc = nullptr;                 // fp32 [C][vd][vh][vw]
  const float* wmap = nullptr;          // fp32 [roi]
  int vd = 0, vh = 0, vw = 0;
  const long long* corner = nullptr;    // [n] voxel offsets (oz vh + oy) vw + ox
};

// decoder stage k (0, 1) runs channel LayerNorm + GELU inside the product's epilogue: no fp32 tensor between the two stages
bool dec_fused(const DecStage& d) { return d.cp == 128 && up(d.cout, 32) <= 128; }

// ---- taps (amx_vit_forward_taps): where every named intermediate of a forward at batch n lives while it is valid.  A tap is one byte
// range, or two that are handed out back to back ([hi plane | lo plane], [scale | shift]); nb == 0: one range.  (The size query builds
// the table on a plan without a base: only the sizes mean anything there.)  The forward states a tap as (kind, index); its name is
// written here alone, %d = the tokenizer stage, block or decoder stage.
enum TapKind {
  T_H0, T_P0, T_RAW1, T_SS1, T_A1, T_RAW2, T_SS2, T_RAWS, T_SSS, T_H, T_P, T_TOKENS,
  T_LN1, T_ATTN, T_LN_ATTN, T_TOK1, T_LN2, T_HD, T_LN_MLP, T_TOK2,
  T_DLN, T_DRAW, T_DIN, T_DMEAN, T_Y
};
const char* const kTapName[] = {"h0", "p0", "s%d.raw1", "s%d.ss1", "s%d.a1", "s%d.raw2", "s%d.ss2", "s%d.raws", "s%d.sss", "s%d.h", "s%d.p", "tokens",
                                "b%d.ln1", "b%d.attn", "b%d.ln_attn", "b%d.tok1", "b%d.ln2", "b%d.hd", "b%d.ln_mlp", "b%d.tok2",
                                "d.ln", "d%d.raw", "d%d.in", "d.mean", "y"};
struct TapSrc {
  int kind, idx;
  std::string name;
  const void *a, *b;      // the range(s)
  size_t na, nb;
  size_t bytes() const { return na + nb; }
};
struct TapReq { amx_vit_tap* req; TapSrc src; };      // a request and the table entry it names, resolved before the first launch
typedef std::vector<TapReq> TapSet;

std::vector<TapSrc> tap_table(const amx_vit* h, int n, const Plan& P, int nb, const float* d_y) {
  std::vector<TapSrc> t;
  const amx_vit_cfg& c = h->cfg;
  const int E = h->E, Ep = h->Ep, T = h->T, V = h->V, hid = h->hidden;
  const size_t M = (size_t)n * T;
  auto two = [&](int kind, int idx, const void* a, const void* b, size_t each, bool pair = true) {
    char name[32];
    snprintf(name, sizeof name, kTapName[kind], idx);
    t.push_back({kind, idx, name, a, pair ? b : nullptr, each, pair ? each : 0});
  };
  auto one = [&](int kind, int idx, const void* a, size_t na) { two(kind, idx, a, nullptr, na, false); };
  size_t vox = (size_t)V * 512;
  two(T_H0, 0, P.h_hi[0], P.h_lo[0], n * vox * 32 * 2, c.stem_split != 0);
  two(T_P0, 0, P.p_hi[0], P.p_lo[0], n * (vox / 8) * 32 * 2);
  for (int k = 0; k < 3; ++k) {
    const size_t C = kStageC[k + 1], vo = vox / 8;
    one(T_RAW1, k, P.raw1, n * vo * C * 4);
    two(T_SS1, k, P.sc[0], P.sh[0], n * C * 4);
    two(T_A1, k, P.a1_hi, P.a1_lo, n * vo * C * 2);
    one(T_RAW2, k, P.raw2, n * vo * C * 4);
    two(T_SS2, k, P.sc[1], P.sh[1], n * C * 4);
    one(T_RAWS, k, P.raws, n * vo * C * 4);
    two(T_SSS, k, P.sc[2], P.sh[2], n * C * 4);
    two(T_H, k, P.h_hi[k + 1], P.h_lo[k + 1], n * vo * C * 2);
    if (k < 2) two(T_P, k, P.p_hi[k + 1], P.p_lo[k + 1], n * (vo / 8) * C * 2);
    vox = vo;
  }
  one(T_TOKENS, 0, P.tok, M * E * 4);
  for (int b = 0; b < nb; ++b) {
    one(T_LN1, b, P.A1, M * Ep * 2);
    one(T_ATTN, b, P.AO, M * E * 4);
    one(T_LN_ATTN, b, P.A1, M * Ep * 2);
    one(T_TOK1, b, P.tok, M * E * 4);
    one(T_LN2, b, P.A1, M * Ep * 2);
    one(T_HD, b, P.Hd, M * up(hid, 16) * 2);
    one(T_LN_MLP, b, P.A2, M * up(hid, 32) * 2);
    one(T_TOK2, b, P.tok, M * E * 4);
  }
  size_t rows = (size_t)n * V;
  two(T_DLN, 0, P.Ad_hi[0], P.Ad_lo[0], rows * Ep * 2, c.decoder_split != 0);
  for (int k = 0; k < 2; ++k) {
    const DecStage& d = h->dec[k];
    rows *= 8;
    if (!dec_fused(d)) one(T_DRAW, k, P.rawd[k], rows * d.cout * 4);
    two(T_DIN, k + 1, P.Ad_hi[k + 1], P.Ad_lo[k + 1], rows * up(d.cout, 32) * 2, c.decoder_split != 0);
  }
  if (c.out_norm == 1) one(T_DMEAN, 0, P.mean, (size_t)n * c.num_classes * 4);
  one(T_Y, 0, d_y, rows * 8 * c.num_classes * 4);
  return t;
}

const TapSrc* tap_find(const std::vector<TapSrc>& t, const char* name) {
  for (const auto& e : t)
    if (e.name == name) return &e;
  return nullptr;
}

// The launch schedule of one forward of n roi-sized samples, one method per step; every argument has been checked by the entry.  `ts`
// (amx_vit_forward_taps): after the launch that produces a named buffer, the requested copies of it are enqueued on the same stream and the
// launch's instance name is written into the request -- no launch is added, moved or routed differently.  Null: no name is formatted at all.
struct VitForward {
  const amx_vit* const h;
  const amx_vit_cfg& c;
  const Plan& P;
  const VitOut& out;
  const TapSet* const ts;
  const hipStream_t st;
  const int n, E, Ep, T, V, hid, M, nreg;       // M: token rows of the batch
  void *Qp, *Kp, *Vt;                           // the attention kernel's f16 operands inside P.att, and their padded extents
  int att_npad, att_nblk;
  amx::VitLaunchInfo li0{}, li1{};
  amx::VitLaunchInfo *const i0, *const i1;      // what a launcher reports into: null without taps

  VitForward(const amx_vit* h_, const Plan& P_, int n_, hipStream_t st_, const VitOut& out_, const TapSet* ts_)
      : h(h_), c(h_->cfg), P(P_), out(out_), ts(ts_), st(st_), n(n_), E(h_->E), Ep(h_->Ep), T(h_->T), V(h_->V), hid(h_->hidden), M(n_ * h_->T),
        nreg(h_->cfg.num_register_tokens), i0(ts_ ? &li0 : nullptr), i1(ts_ ? &li1 : nullptr) {
    amx::attention_operands(P.att, n, c.heads, T, &Qp, &Kp, &Vt, &att_npad, &att_nblk);
  }

  int run(const float* d_x, int n_blocks) {      // n_blocks: 0 .. depth
    int e = stem(d_x);
    for (int k = 0; k < 3 && !e; ++k) e = stage(k);
    if (!e) e = embed();
    if (!e && n_blocks > 0) e = clear_attention_operands();
    for (int b = 0; b < n_blocks && !e; ++b) e = block(b);
    if (!e) e = final_norm();
    for (int k = 0; k < 3 && !e; ++k) e = decoder_stage(k);
    return e;
  }
  // the buffer of tap (kind, idx) has just been produced by `route`
  hipError_t tap(int kind, int idx, const char* route) const {
    if (!ts) return hipSuccess;
    for (const TapReq& q : *ts) {
      const TapSrc& s = q.src;
      if (s.kind != kind || s.idx != idx) continue;
      snprintf(q.req->route, sizeof q.req->route, "%s", route);
      if (!q.req->d_dst) continue;
      hipError_t e = hipMemcpyAsync(q.req->d_dst, s.a, s.na, hipMemcpyDeviceToDevice, st);
      if (e == hipSuccess && s.nb) e = hipMemcpyAsync((char*)q.req->d_dst + s.na, s.b, s.nb, hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  // a launch, then the tap of what it produced (route null: the instance the launcher reported)
  hipError_t tapped(hipError_t launched, int kind, int idx, const char* route = nullptr) const {
    return launched != hipSuccess ? launched : tap(kind, idx, route ? route : li0.name);
  }
  // ---- parameter builders.  A product's operand and packed-weight fields: M rows of A (hi [+ lo], lda halves each) times W; the epilogue's are the caller's
  static amx::GemmParams product(const char* a_hi, const char* a_lo, int lda, int M, const Packed& w) {
    amx::GemmParams g{};
    g.a_hi = a_hi; g.a_lo = a_lo; g.lda = lda; g.M = M;
    g.w_hi = w.hi; g.w_lo = w.lo; g.ntiles = w.ntiles; g.KS = w.KS;
    return g;
  }
  // a conv of the tokenizer: input planes [n][D][H][W][Cin] -> raw [n][D / stride]...[Cout] (+ bias), partial statistics into P.stats
  amx::TokConvParams conv(const char* x_hi, const char* x_lo, int D, int H, int W, int Cin, int stride, int Cout, const Packed& w, const float* bias,
                          float* raw) const {
    amx::TokConvParams cp{};
    cp.x_hi = x_hi; cp.x_lo = x_lo; cp.N = n; cp.D = D; cp.H = H; cp.W = W; cp.Cin = Cin;
    cp.Do = D / stride; cp.Ho = H / stride; cp.Wo = W / stride; cp.Cout = Cout;
    cp.w_hi = w.hi; cp.w_lo = w.lo; cp.bias = bias; cp.raw = raw; cp.stats = P.stats;
    return cp;
  }
  struct LnIn { const void* p; int f16, ld, C; };      // the rows to normalise: fp32 or f16, ld elements apart, C columns
  struct LnOut { char *hi, *lo; int ld; };             // f16 operand rows, ld halves each (lo null: no remainder plane)
  // LayerNorm (w null: a plain conversion) [+ GELU] of `rows` whole rows
  hipError_t ln_whole_rows(LnIn in, const float* w, const float* b, float eps, int rows, int gelu, LnOut o) {
    return amx::launch_ln_rows(in.p, in.f16, in.ld, in.C, w, b, eps, rows, rows, rows, 0, gelu, o.hi, o.lo, o.ld, st, i0);
  }
  // ---- tokenizer
  int stem(const float* d_x) {
    const int D0 = c.grid_d * 8, H0 = c.grid_h * 8, W0 = c.grid_w * 8;
    amx::TokStemParams sp{};         // pass 0: statistics; pass 1: normalised output and its average
    sp.x = d_x; sp.N = n; sp.D = D0; sp.H = H0; sp.W = W0;
    sp.w_hi = h->stem_w.hi; sp.w_lo = h->stem_w.lo; sp.bias = h->stem_b; sp.stats = P.stats;
    sp.scale = P.sc[0]; sp.shift = P.sh[0]; sp.slope = 0.01f;
    sp.h_hi = P.h_hi[0]; sp.h_lo = c.stem_split ? P.h_lo[0] : nullptr; sp.p_hi = P.p_hi[0]; sp.p_lo = P.p_lo[0];
    AMX_HIP(amx::launch_tokstem(sp, 0, st));
    AMX_HIP(amx::launch_tok_finalize(P.stats, n, amx::tokstem_slots(D0, H0, W0), 32, (long long)D0 * H0 * W0, h->stem_nw, h->stem_nb, c.in_eps, P.sc[0], P.sh[0], st));
    AMX_HIP(tapped(amx::launch_tokstem(sp, 1, st, i0), T_H0, 0));
    AMX_HIP(tap(T_P0, 0, li0.name));
    return AMX_OK;
  }
  // InstanceNorm statistics of the conv that `cp` just ran -> (scale, shift) set `set`
  hipError_t finalize(const amx::TokConvParams& cp, const float* gamma, const float* beta, int set) {
    return amx::launch_tok_finalize(P.stats, n, amx::tokconv_slots(cp), cp.Cout, (long long)cp.Do * cp.Ho * cp.Wo, gamma, beta, c.in_eps, P.sc[set], P.sh[set], st);
  }
  // stage k: lrelu(IN(conv2(lrelu(IN(conv1(x))))) + IN(skip(avgpool(x)))) at half the input's extent, and its average for the next stage
  int stage(int k) {
    const Stage& s = h->st[k];
    const int Dk = c.grid_d * 8 >> k, Hk = c.grid_h * 8 >> k, Wk = c.grid_w * 8 >> k, Do = Dk / 2, Ho = Hk / 2, Wo = Wk / 2;
    // conv1: stride 2 from the stage input
    const amx::TokConvParams c1 = conv(P.h_hi[k], (k == 0 && !c.stem_split) ? nullptr : P.h_lo[k], Dk, Hk, Wk, s.cin, 2, s.cout, s.c1, s.c1b, P.raw1);
    AMX_HIP(tapped(amx::launch_tokconv(c1, 27, 2, st, i0), T_RAW1, k));
    AMX_HIP(tapped(finalize(c1, s.n1w, s.n1b, 0), T_SS1, k, "tok_finalize"));
    AMX_HIP(tapped(amx::launch_tok_apply(P.raw1, n, (long long)Do * Ho * Wo, s.cout, P.sc[0], P.sh[0], 0.01f, P.a1_hi, P.a1_lo, st), T_A1, k, "tok_apply"));
    const amx::TokConvParams c2 = conv(P.a1_hi, P.a1_lo, Do, Ho, Wo, s.cout, 1, s.cout, s.c2, s.c2b, P.raw2);
    AMX_HIP(tapped(amx::launch_tokconv(c2, 27, 1, st, i0), T_RAW2, k));
    AMX_HIP(tapped(finalize(c2, s.n2w, s.n2b, 1), T_SS2, k, "tok_finalize"));
    // skip: 1x1x1 conv of the average-pooled stage input (no bias)
    const amx::TokConvParams sk = conv(P.p_hi[k], P.p_lo[k], Do, Ho, Wo, s.cin, 1, s.cout, s.sk, nullptr, P.raws);
    AMX_HIP(tapped(amx::launch_tokconv(sk, 1, 1, st, i0), T_RAWS, k));
    AMX_HIP(tapped(finalize(sk, s.snw, s.snb, 2), T_SSS, k, "tok_finalize"));
    AMX_HIP(amx::launch_tok_combine(P.raw2, P.raws, n, Do, Ho, Wo, s.cout, P.sc[1], P.sh[1], P.sc[2], P.sh[2], 0.01f, P.h_hi[k + 1], P.h_lo[k + 1],
                                    k < 2 ? P.p_hi[k + 1] : nullptr, k < 2 ? P.p_lo[k + 1] : nullptr, st));
    AMX_HIP(tap(T_H, k, "tok_combine"));
    if (k < 2) AMX_HIP(tap(T_P, k, "tok_combine"));
    return AMX_OK;
  }
  // token projection (+ bias + position embedding) behind the register tokens of every sample
  int embed() {
    amx::GemmParams g = product(P.h_hi[3], P.h_lo[3], kStageC[3], n * V, h->tokproj);
    g.Nreal = E; g.bias = h->tokproj_b; g.out = P.tok; g.ldo = E; g.V = V; g.nreg = nreg; g.pos = h->pos;
    AMX_HIP(amx::launch_gemm(g, amx::EPI_TOKENS, st, i0));
    AMX_HIP(tapped(amx::launch_place_registers(h->regs, nreg, E, T, n, P.tok, st), T_TOKENS, 0));
    return AMX_OK;
  }
  // ---- EVA blocks
  // padding of the operand buffers (token rows / keys beyond T, feature columns beyond head_dim) is zero and never written again
  int clear_attention_operands() {
    AMX_HIP(hipMemsetAsync(P.att, 0, amx::attention_scratch_bytes(n, c.heads, T), st));
    return AMX_OK;
  }
  // The q | k (EPI_QK) or v (EPI_VT) projection of the rows in P.A1.  It writes the attention kernel's f16 operands itself (bias, per-head
  // LayerNorm, rotary embedding, fragment layouts in the epilogue): no fp32 q / k / v tensors, no separate preparation pass
  amx::GemmParams attention_operand(const Block& b, const Packed& w, const float* bias, void* dst) const {
    amx::GemmParams g = product(P.A1, nullptr, Ep, M, w);
    g.Nreal = w.ntiles * 16; g.bias = bias; g.out = dst; g.ldo = 0;
    g.att_eps = 1e-5f; g.qscale = 1.4426950408889634f / sqrtf((float)h->hd); g.rope = h->rope; g.T = T; g.n_prefix = nreg; g.heads = c.heads;
    g.hd = h->hd; g.npad = att_npad; g.nblk_pad = att_nblk; g.Qp = Qp; g.Kp = Kp; g.Vt = Vt; g.Cp = 80;
    g.qnw = c.qk_norm ? b.qnw : nullptr; g.qnb = b.qnb; g.knw = c.qk_norm ? b.knw : nullptr; g.knb = b.knb;
    return g;
  }
  // tok += gamma * (rows x W + bias): the residual products behind attention and MLP
  hipError_t residual(const char* rows, int lda, const Packed& w, const float* bias, const float* gamma) {
    amx::GemmParams g = product(rows, nullptr, lda, M, w);
    g.Nreal = E; g.bias = bias; g.gamma = gamma; g.out = P.tok; g.ldo = E;
    return amx::launch_gemm(g, amx::EPI_RESID, st, i0);
  }
  int block(int bi) {
    const Block& b = h->blk[bi];
    // ---- attention
    AMX_HIP(tapped(ln_whole_rows({P.tok, 0, E, E}, b.n1w, b.n1b, 1e-6f, M, 0, {P.A1, nullptr, Ep}), T_LN1, bi));
    AMX_HIP(amx::launch_gemm(attention_operand(b, b.qk, b.qkb, Qp), amx::EPI_QK, st, i0));
    AMX_HIP(amx::launch_gemm(attention_operand(b, b.v, b.vb, Vt), amx::EPI_VT, st, i1));
    char group[sizeof li0.name + sizeof li1.name + 16] = "";      // the operand buffers are not tapped: one group
    if (ts) snprintf(group, sizeof group, "%s + %s + attn_fwd", li0.name, li1.name);
    AMX_HIP(tapped(amx::launch_attention_fwd(Qp, Kp, Vt, n, T, c.heads, h->hd, P.AO, st), T_ATTN, bi, group));
    AMX_HIP(tapped(ln_whole_rows({P.AO, 0, E, E}, c.scale_attn_inner ? b.anw : nullptr, b.anb, 1e-5f, M, 0, {P.A1, nullptr, Ep}), T_LN_ATTN, bi));
    AMX_HIP(tapped(residual(P.A1, Ep, b.proj, b.projb, b.g1), T_TOK1, bi));
    // ---- SwiGLU MLP
    AMX_HIP(tapped(ln_whole_rows({P.tok, 0, E, E}, b.n2w, b.n2b, 1e-6f, M, 0, {P.A1, nullptr, Ep}), T_LN2, bi));
    amx::GemmParams g = product(P.A1, nullptr, Ep, M, b.fc1);
    g.Nreal = 2 * up(hid, 16); g.bias = b.fc1b; g.out = P.Hd; g.ldo = up(hid, 16);
    AMX_HIP(tapped(amx::launch_gemm(g, amx::EPI_SWIGLU, st, i0), T_HD, bi));
    AMX_HIP(tapped(ln_whole_rows({P.Hd, 1, up(hid, 16), hid}, b.mnw, b.mnb, 1e-6f, M, 0, {P.A2, nullptr, up(hid, 32)}), T_LN_MLP, bi));
    AMX_HIP(tapped(residual(P.A2, up(hid, 32), b.fc2, b.fc2b, b.g2), T_TOK2, bi));
    return AMX_OK;
  }
  // ---- final norm + decoder
  // the final norm drops the register tokens: output row r of sample s is token row s T + nreg + r
  int final_norm() {
    AMX_HIP(tapped(amx::launch_ln_rows(P.tok, 0, E, E, h->fnw, h->fnb, 1e-6f, /* M */ n * V, /* rows_out */ V, /* rows_in */ T, /* skip */ nreg,
                                       /* gelu */ 0, P.Ad_hi[0], P.Ad_lo[0], Ep, st, i0), T_DLN, 0));
    return AMX_OK;
  }
  // the product of decoder stage k (ConvTranspose3d, kernel 2, stride 2) on `rows` of its operand rows from row0; where the result goes is the caller's
  amx::GemmParams dec_product(int k, long long row0, long long rows) const {
    const DecStage& d = h->dec[k];
    const int lda = up(d.cin, 32);
    amx::GemmParams g = product(P.Ad_hi[k] + row0 * lda * 2, P.Ad_lo[k] ? P.Ad_lo[k] + row0 * lda * 2 : nullptr, lda, (int)rows, d.w);
    g.Nreal = 8 * d.cp; g.bias = d.bias; g.ldo = d.cout; g.Cp = d.cp; g.Creal = d.cout;
    g.gd = c.grid_d << k; g.gh = c.grid_h << k; g.gw = c.grid_w << k;
    return g;
  }
  int decoder_stage(int k) {
    const long long rows = ((long long)n * V) << (3 * k);      // operand rows of the stage; it writes 8 times as many
    if (k < 2) return dec_fused(h->dec[k]) ? scatter_ln(k, rows) : scatter_then_ln(k, rows);
    if (c.out_norm == 1)
      if (int e = demean(rows)) return e;
    return out.acc ? planar_acc(rows) : planar(rows);
  }
  // channel LayerNorm + GELU fused into the product: the next stage's operand rows come straight out, no fp32 tensor between the two
  int scatter_ln(int k, long long rows) {
    const DecStage& d = h->dec[k];
    amx::GemmParams g = dec_product(k, 0, rows);
    g.out = P.Ad_hi[k + 1]; g.out_lo = P.Ad_lo[k + 1]; g.ldo = up(d.cout, 32); g.lnw = d.lnw; g.lnb = d.lnb; g.eps = 1e-6f;
    AMX_HIP(tapped(amx::launch_gemm(g, amx::EPI_SCATTER_LN, st, i0), T_DIN, k + 1));
    return AMX_OK;
  }
  int scatter_then_ln(int k, long long rows) {
    const DecStage& d = h->dec[k];
    amx::GemmParams g = dec_product(k, 0, rows);
    g.out = P.rawd[k];
    AMX_HIP(tapped(amx::launch_gemm(g, amx::EPI_SCATTER, st, i0), T_DRAW, k));
    AMX_HIP(tapped(ln_whole_rows({P.rawd[k], 0, d.cout, d.cout}, d.lnw, d.lnb, 1e-6f, (int)(rows * 8), 1, {P.Ad_hi[k + 1], P.Ad_lo[k + 1], up(d.cout, 32)}), T_DIN, k + 1));
    return AMX_OK;
  }
  // ChannelDemean: the mean of every output channel follows from the column means of the last stage's input
  int demean(long long rows) {
    const DecStage& d = h->dec[2];
    AMX_HIP(amx::launch_colsum(P.Ad_hi[2], P.Ad_lo[2], up(d.cin, 32), d.cin, n, (int)(rows / n), kColChunks, P.colsum, st));
    AMX_HIP(tapped(amx::launch_demean(P.colsum, kColChunks, up(d.cin, 32), d.cin, rows / n, d.w_raw, d.cout, d.bias, n, P.mean, st), T_DMEAN, 0, "colsum + demean"));
    return AMX_OK;
  }
  // planar fp32 output written by the product kernel itself
  int planar(long long rows) {
    amx::GemmParams g = dec_product(2, 0, rows);
    g.out = out.y; g.sub = c.out_norm == 1 ? P.mean : nullptr;
    AMX_HIP(tapped(amx::launch_gemm(g, amx::EPI_PLANAR, st, i0), T_Y, 0));
    return AMX_OK;
  }
  // sliding window: one product per window, in window order (overlapping windows are ordered by the stream), blended into the accumulator
  int planar_acc(long long rows) {
    const long long wrows = rows / n;
    for (int i = 0; i < n; ++i) {
      amx::GemmParams g = dec_product(2, i * wrows, wrows);
      g.wmap = out.wmap; g.acc_sc = (long long)out.vd * out.vh * out.vw; g.acc_sz = (long long)out.vh * out.vw; g.acc_sy = out.vw;
      g.out = out.acc + out.corner[i]; g.sub = c.out_norm == 1 ? P.mean + (size_t)i * h->dec[2].cout : nullptr;      // ChannelDemean stays per window
      AMX_HIP(amx::launch_gemm(g, amx::EPI_PLANAR_ACC, st));
    }
    return AMX_OK;
  }
};

// ---- sliding-window route -----------------------------------------------------------------------------------------------------
constexpr int kVitMaxWindows = 16;
struct VitCorners { long long off[kVitMaxWindows]; };

// win[i][z][y][x] = vol[corner i + (z vh + y) vw + x]: the roi-sized batch the tokenizer reads (1 / 32 of what the decoder writes).
// A thread moves four voxels of a row (rw is a multiple of 16); the corner may sit at any x, so the loads are scalar.
__global__ __launch_bounds__(256) void vit_gather_windows_kernel(const float* __restrict__ vol, int vh, int vw, VitCorners c, int rd, int rh,
                                                                 int rw, float* __restrict__ win) {
  const long long quads = (long long)rd * rh * (rw >> 2);
  const float* src = vol + c.off[blockIdx.y];
  float4* dst = (float4*)(win + (long long)blockIdx.y * rd * rh * rw);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < quads; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % (rw >> 2)) * 4;
    const long long r = i / (rw >> 2);
    const int y = (int)(r % rh), z = (int)(r / rh);
    const float* s = src + ((long long)z * vh + y) * vw + x;
    dst[i] = make_float4(s[0], s[1], s[2], s[3]);
  }
}

struct VitWindowsWs {          // [gathered windows | the forward's plan]
  size_t gather, total;
};
VitWindowsWs windows_ws(const amx_vit* h, int n) {
  VitWindowsWs w;
  w.gather = ((size_t)n * h->V * 512 * sizeof(float) + 255) & ~(size_t)255;
  w.total = w.gather + make_plan(h, n, nullptr).total;
  return w;
}

// every check of amx_vit_forward_windows but the offsets'
int windows_check(const amx_vit* h, int vd, int vh, int vw, int n_windows, const void* d_ws, size_t ws_bytes) {
  if (!h->loaded) return fail(AMX_ERR_NOT_LOADED, "vit: windows before amx_vit_load");
  if (n_windows < 1 || n_windows > kVitMaxWindows) return fail(AMX_ERR_INVALID, "vit: 1 <= n_windows <= %d (got %d)", kVitMaxWindows, n_windows);
  const amx_vit_cfg& c = h->cfg;
  if (vd < c.grid_d * 8 || vh < c.grid_h * 8 || vw < c.grid_w * 8)
    return fail(AMX_ERR_SHAPE, "vit: volume %d x %d x %d is smaller than the roi %d x %d x %d: pad it first", vd, vh, vw, c.grid_d * 8, c.grid_h * 8,
                c.grid_w * 8);
  if ((long long)vd * vh * vw >= (1LL << 40) / c.num_classes) return fail(AMX_ERR_SHAPE, "vit: volume %d x %d x %d is too large", vd, vh, vw);
  if (c.out_norm != 0 && c.out_norm != 1) return fail(AMX_ERR_INVALID, "vit: out_norm %d is not applied by the engine", c.out_norm);
  const size_t need = windows_ws(h, n_windows).total;
  if (ws_bytes < need || ((uintptr_t)d_ws & 255))
    return fail(AMX_ERR_WORKSPACE, "vit: workspace needs %zu bytes, 256-byte aligned (got %zu)", need, ws_bytes);
  return AMX_OK;
}

int forward_windows(const amx_vit* h, const float* d_vol, int vd, int vh, int vw, int n, const int* offsets_zyx, const float* d_wmap, float* d_acc,
                    void* d_ws, size_t ws_bytes, hipStream_t st) {
  if (int rc = windows_check(h, vd, vh, vw, n, d_ws, ws_bytes)) return rc;
  const amx_vit_cfg& c = h->cfg;
  const int rd = c.grid_d * 8, rh = c.grid_h * 8, rw = c.grid_w * 8;
  VitCorners cn{};
  if (int rc = amx::sw_window_offsets(vd, vh, vw, rd, rh, rw, n, offsets_zyx, cn.off)) return rc;
  // ---- launches
  float* win = (float*)d_ws;
  const Plan P = make_plan(h, n, (char*)d_ws + windows_ws(h, n).gather);
  const long long quads = (long long)rd * rh * (rw / 4);
  const int blocks = (int)((quads + 255) / 256 > 2048 ? 2048 : (quads + 255) / 256);
  hipLaunchKernelGGL(vit_gather_windows_kernel, dim3(blocks, n), dim3(256), 0, st, d_vol, vh, vw, cn, rd, rh, rw, win);
  AMX_HIP(hipGetLastError());
  VitOut out;
  out.acc = d_acc; out.wmap = d_wmap; out.vd = vd; out.vh = vh; out.vw = vw; out.corner = cn.off;
  return VitForward(h, P, n, st, out, nullptr).run(win, c.depth);
}

// amx_vit_forward and amx_vit_forward_taps: a plain forward is a forward with zero taps.  Every refusal comes before the first launch.
int forward_checked(const amx_vit* h, const float* d_x, float* d_y, int n, void* d_ws, size_t ws_bytes, int n_blocks, amx_vit_tap* taps, int n_taps,
                    hipStream_t st) {
  if (!h || !d_x || !d_y || !d_ws || n_taps < 0 || (n_taps && !taps)) return fail(AMX_ERR_INVALID, "null argument");
  if (!h->loaded) return fail(AMX_ERR_NOT_LOADED, "vit: forward before amx_vit_load");
  if (n < 1) return fail(AMX_ERR_INVALID, "vit: batch %d", n);
  if ((uintptr_t)d_ws & 255) return fail(AMX_ERR_WORKSPACE, "vit: workspace must be 256-byte aligned");
  const Plan P = make_plan(h, n, (char*)d_ws);
  if (ws_bytes < P.total) return fail(AMX_ERR_WORKSPACE, "vit: workspace needs %zu bytes (got %zu)", P.total, ws_bytes);
  const int nb = n_blocks < 0 || n_blocks > h->cfg.depth ? h->cfg.depth : n_blocks;
  TapSet ts;
  const std::vector<TapSrc> table = n_taps ? tap_table(h, n, P, nb, d_y) : std::vector<TapSrc>();
  for (int i = 0; i < n_taps; ++i) {
    if (!taps[i].name) return fail(AMX_ERR_INVALID, "vit: tap %d has no name", i);
    const TapSrc* s = tap_find(table, taps[i].name);
    if (!s) return fail(AMX_ERR_INVALID, "vit: no tap named %s in this forward (%d blocks)", taps[i].name, nb);
    if (taps[i].d_dst && taps[i].bytes < s->bytes())
      return fail(AMX_ERR_WORKSPACE, "vit: tap %s needs %zu bytes (got %zu)", taps[i].name, s->bytes(), taps[i].bytes);
    taps[i].route[0] = 0;
    ts.push_back({&taps[i], *s});
  }
  const VitOut out{d_y};
  return VitForward(h, P, n, st, out, n_taps ? &ts : nullptr).run(d_x, nb);
}

}  // namespace

extern "C" {

size_t amx_vit_workspace_bytes(const amx_vit_t* h, int n) {
  if (!h || n < 1) return 0;
  return make_plan(h, n, nullptr).total;
}

int amx_vit_forward(amx_vit_t* h, const float* d_x, float* d_y, int n, void* d_ws, size_t ws_bytes, int n_blocks, void* stream) {
  return forward_checked(h, d_x, d_y, n, d_ws, ws_bytes, n_blocks, nullptr, 0, (hipStream_t)stream);
}

size_t amx_vit_tap_bytes(const amx_vit_t* h, int n, const char* name) {
  if (!h || n < 1 || !name) return 0;
  const std::vector<TapSrc> t = tap_table(h, n, make_plan(h, n, nullptr), h->cfg.depth, nullptr);
  const TapSrc* s = tap_find(t, name);
  return s ? s->bytes() : 0;
}

int amx_vit_forward_taps(amx_vit_t* h, const float* d_x, float* d_y, int n, void* d_ws, size_t ws_bytes, int n_blocks, amx_vit_tap* taps,
                         int n_taps, void* stream) {
  return forward_checked(h, d_x, d_y, n, d_ws, ws_bytes, n_blocks, taps, n_taps, (hipStream_t)stream);
}

size_t amx_vit_windows_workspace_bytes(const amx_vit_t* h, int n_windows) {
  if (!h || n_windows < 1 || n_windows > kVitMaxWindows) return 0;
  return windows_ws(h, n_windows).total;
}

int amx_vit_forward_windows(amx_vit_t* h, const float* d_vol, int vd, int vh, int vw, int n_windows, const int* offsets_zyx,
                            const float* d_wmap, float* d_acc, void* d_ws, size_t ws_bytes, void* stream) {
  if (!h || !d_vol || !offsets_zyx || !d_wmap || !d_acc || !d_ws) return fail(AMX_ERR_INVALID, "null argument");
  return forward_windows(h, d_vol, vd, vh, vw, n_windows, offsets_zyx, d_wmap, d_acc, d_ws, ws_bytes, (hipStream_t)stream);
}

size_t amx_vit_sliding_window_workspace_bytes(const amx_vit_t* h, int n_batch) { return amx_vit_windows_workspace_bytes(h, n_batch); }

int amx_vit_sliding_window(amx_vit_t* h, const float* d_vol, int vd, int vh, int vw, double overlap, int mode, double sigma_scale, int n_batch,
                           int out_kind, const float* d_w, const float* d_b, int classes, float* d_acc, float* d_cnt, void* d_out, void* d_ws,
                           size_t ws_bytes, void* stream) {
  if (!h || !d_vol || !d_acc || !d_cnt || !d_ws) return fail(AMX_ERR_INVALID, "null argument");
  const amx_vit_cfg& c = h->cfg;
  amx::SwNet net{"amx_vit_sliding_window", "vit: ", c.num_classes, kVitMaxWindows, {c.grid_d * 8, c.grid_h * 8, c.grid_w * 8}, 0};      // one stream
  net.check = [&](int) { return windows_check(h, vd, vh, vw, n_batch, d_ws, ws_bytes); };
  net.run = [&](int nw, const int* offs, int, hipStream_t st) {
    return forward_windows(h, d_vol, vd, vh, vw, nw, offs, h->sw_map.map, d_acc, d_ws, ws_bytes, st);
  };
  return amx::sw_run(net, h->sw_map, nullptr, vd, vh, vw, overlap, mode, sigma_scale, n_batch, out_kind, d_w, d_b, classes, d_acc, d_cnt, d_out,
                     (hipStream_t)stream);
}

}  // extern "C"
