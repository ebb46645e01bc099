// anatomix_amd -- the second stage of the registration, downstream of amx_regsolve.hip:
//   create_warp / run_instance_opt   anatomix/registration/instance_optimization.py:225-399 (Adam on a displacement grid)
//   the driver's warp                anatomix/registration/run_convex_adam_with_network_feats.py:238-266
// fp32 throughout, batch 1, planar [C][h][w][d], on the caller's stream without host synchronisation.  Streaming / stencil /
// gather work, no MFMA.  One Adam iteration is four launches: smooth (weight -> disp_sample), sample + gradient (the data
// term's grid_sample forward and backward and the regulariser's gradient in one pass over the voxels), smooth again (the
// three box passes are symmetric, so their adjoint is the same kernel) and the update.  No fused multiply-add contraction
// (see the pragma), as in the solver.
#include <math.h>
#include <stdio.h>

#include "amx_device.h"
#include "amx_launch.h"
#include "amx_stream.h"

#pragma clang fp contract(off)

namespace amx {

// ---- three zero-padded box-3 passes of a field in one launch ------------------------------------------------------------
// An 8 x 8 x 32 output tile with a 3-voxel halo lives in LDS; pass m reads frame A and writes the region that is m voxels
// inside the frame into frame B, with ZERO wherever the position lies outside the volume (each pass of apply_avg_pool3d pads
// its own input with zeros: three truncated passes are not one 7-tap filter near the border).  Each pass sums as
// box_filter_kernel does -- 3 x 3 plane sums in (y, x) order, then the three planes in z order, then / 27 -- so the result is
// the three amx_box_filter3d launches' bit for bit.
constexpr int kSmZ = 8, kSmY = 8, kSmX = 32, kSmHalo = 3;
constexpr int kSmLZ = kSmZ + 2 * kSmHalo, kSmLY = kSmY + 2 * kSmHalo, kSmLX = kSmX + 2 * kSmHalo, kSmLXP = kSmLX | 1;
constexpr int kSmFrame = kSmLZ * kSmLY * kSmLXP;

template <int M, bool LAST>
__device__ __forceinline__ void smooth_pass(const float* __restrict__ a, float* __restrict__ b, int fz, int fy, int fx, int H,
                                            int W, int D, float* __restrict__ out) {
  constexpr int NY = kSmLY - 2 * M, NX = kSmLX - 2 * M;
  for (int col = threadIdx.x; col < NY * NX; col += 256) {
    const int ly = M + col / NX, lx = M + col % NX;
    const int gy = fy + ly, gx = fx + lx;
    const bool cin = gy >= 0 && gy < W && gx >= 0 && gx < D;
    float p0 = 0.f, p1 = 0.f;
    for (int lz = M - 1; lz <= kSmLZ - M; ++lz) {
      float ps = 0.f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) ps += a[(lz * kSmLY + ly - 1 + ky) * kSmLXP + lx - 1 + kx];
      if (lz >= M + 1) {
        const int oz = lz - 1, gz = fz + oz;
        const float v = ((p0 + p1) + ps) / 27.f;
        const bool in = cin && gz >= 0 && gz < H;
        if (!LAST) b[(oz * kSmLY + ly) * kSmLXP + lx] = in ? v : 0.f;
        else if (in) out[((long long)gz * W + gy) * D + gx] = v;
      }
      p0 = p1;
      p1 = ps;
    }
  }
}

__global__ __launch_bounds__(256) void instopt_smooth3_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                              int D) {
  __shared__ float frame[2][kSmFrame];
  const long long plane = (long long)H * W * D;
  const int nbx = (D + kSmX - 1) / kSmX, nby = (W + kSmY - 1) / kSmY;
  const int fx = (blockIdx.x % nbx) * kSmX - kSmHalo, fy = ((blockIdx.x / nbx) % nby) * kSmY - kSmHalo,
            fz = (blockIdx.x / (nbx * nby)) * kSmZ - kSmHalo;
  const float* src = in + (long long)blockIdx.y * plane;
  for (int t = threadIdx.x; t < kSmLZ * kSmLY * kSmLX; t += 256) {
    const int lx = t % kSmLX, ly = (t / kSmLX) % kSmLY, lz = t / (kSmLX * kSmLY);
    const int z = fz + lz, y = fy + ly, x = fx + lx;
    frame[0][(lz * kSmLY + ly) * kSmLXP + lx] = (z >= 0 && z < H && y >= 0 && y < W && x >= 0 && x < D) ? src[((long long)z * W + y) * D + x] : 0.f;
  }
  __syncthreads();
  smooth_pass<1, false>(frame[0], frame[1], fz, fy, fx, H, W, D, nullptr);
  __syncthreads();
  smooth_pass<2, false>(frame[1], frame[0], fz, fy, fx, H, W, D, nullptr);
  __syncthreads();
  smooth_pass<3, true>(frame[0], nullptr, fz, fy, fx, H, W, D, out + (long long)blockIdx.y * plane);
}

// ---- sample + gradient --------------------------------------------------------------------------------------------------
struct InstoptCoef {
  float half[3];        // (n - 1) / 2 per axis: disp_sample / half is added to the identity grid (instance_optimization.py:339-357)
  float data[3];        // 2 * 12 / (c h w d) * (n / 2) / ((n - 1) / 2): d loss / d disp_sample from sum_c (s_c - f_c) ds_c / d coord
  float reg[3];         // 2 lambda / (number of elements of that axis' mean)
};

// corner j of a sample: bit 0 = +1 along d (grid_sample's x), bit 1 along w, bit 2 along h
struct Corners {
  int off[8];
  bool in[8];
  float wgt[8];         // trilinear weight
  float dw[3][8];       // its derivative with respect to the (unnormalised) coordinate along h, w, d
};

// unnormalised coordinate of grid_sample(align_corners=False), clamped into [-2, n + 1] (NaN -> -2) so that the integer
// conversion is defined; a clamped coordinate has every corner out of range
__device__ __forceinline__ float sample_coord(float g, int n) {
  const float i = ((g + 1.f) * (float)n - 1.f) / 2.f;
  return fminf(fmaxf(i, -2.f), (float)(n + 1));
}

__device__ __forceinline__ void corners_of(float iz, float iy, float ix, int H, int W, int D, Corners& k) {
  const float fz = floorf(iz), fy = floorf(iy), fx = floorf(ix);
  const int z0 = (int)fz, y0 = (int)fy, x0 = (int)fx;
  const float wz1 = iz - fz, wz0 = (fz + 1.f) - iz, wy1 = iy - fy, wy0 = (fy + 1.f) - iy, wx1 = ix - fx, wx0 = (fx + 1.f) - ix;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int bx = j & 1, by = (j >> 1) & 1, bz = j >> 2;
    const int xx = x0 + bx, yy = y0 + by, zz = z0 + bz;
    k.in[j] = xx >= 0 && xx < D && yy >= 0 && yy < W && zz >= 0 && zz < H;
    k.off[j] = k.in[j] ? (zz * W + yy) * D + xx : 0;
    const float wx = bx ? wx1 : wx0, wy = by ? wy1 : wy0, wz = bz ? wz1 : wz0;
    k.wgt[j] = wx * wy * wz;
    // grid_sampler_3d_backward (zeros padding): the weight of a corner differentiates to -/+ the product of the other two
    k.dw[0][j] = bz ? wx * wy : -(wx * wy);
    k.dw[1][j] = by ? wx * wz : -(wx * wz);
    k.dw[2][j] = bx ? wy * wz : -(wy * wz);
  }
}

// grad_sample = d (loss + reg) / d disp_sample for one voxel per thread, consecutive lanes along d:
//   loss = mean_voxels(mean_c((grid_sample(mov, id + ds / half) - fix)^2) * 12),  reg = lambda * (three means of squared forward differences).
// LOSS: also one partial {sum of squared residuals, three sums of squared differences} per block in partial[4][gridDim.x].
template <bool LOSS>
__global__ __launch_bounds__(256) void instopt_sample_grad_kernel(const float* __restrict__ ds, const float* __restrict__ fix,
                                                                  const float* __restrict__ mov, int C, int H, int W, int D,
                                                                  InstoptCoef cf, float* __restrict__ grad,
                                                                  float* __restrict__ partial) {
  __shared__ float red[LOSS ? 256 : 1];
  const int plane = H * W * D, o = (int)(blockIdx.x * 256 + threadIdx.x);
  const bool live = o < plane;
  float sq = 0.f, rsum[3] = {0.f, 0.f, 0.f};
  if (live) {
    const int x = o % D, y = (o / D) % W, z = o / (D * W);
    const float v[3] = {ds[o], ds[(long long)plane + o], ds[2LL * plane + o]};
    Corners k;
    corners_of(sample_coord(identity_coord(z, H) + v[0] / cf.half[0], H), sample_coord(identity_coord(y, W) + v[1] / cf.half[1], W),
               sample_coord(identity_coord(x, D) + v[2] / cf.half[2], D), H, W, D, k);
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
      const float* m = mov + (long long)c * plane;
      float val[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) val[j] = k.in[j] ? m[k.off[j]] : 0.f;      // out-of-range corners are not loaded
      float s = 0.f, dz = 0.f, dy = 0.f, dx = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s += val[j] * k.wgt[j];
        dz += val[j] * k.dw[0][j];
        dy += val[j] * k.dw[1][j];
        dx += val[j] * k.dw[2][j];
      }
      const float r = s - fix[(long long)c * plane + o];
      acc[0] += r * dz;
      acc[1] += r * dy;
      acc[2] += r * dx;
      if (LOSS) sq += r * r;
    }
    // the regulariser: forward differences along h (stride W D), w (stride D), d (stride 1) of every channel
    const int pos[3] = {z, y, x}, ext[3] = {H, W, D}, stride[3] = {W * D, D, 1};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float* f = ds + (long long)a * plane;
      float g = cf.data[a] * acc[a];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        float t = 0.f;
        if (pos[e] > 0) t += v[a] - f[o - stride[e]];
        if (pos[e] < ext[e] - 1) {
          const float fd = f[o + stride[e]] - v[a];
          t -= fd;
          if (LOSS) rsum[e] += fd * fd;
        }
        g += cf.reg[e] * t;
      }
      grad[(long long)a * plane + o] = g;
    }
  }
  if (LOSS) {
    const float vals[4] = {sq, rsum[0], rsum[1], rsum[2]};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float r = block_tree_sum<float, 256>(vals[q], red);
      if (threadIdx.x == 0) partial[(long long)q * gridDim.x + blockIdx.x] = r;
    }
  }
}

// second stage of the loss: one block adds the per-block partials in a fixed order (double), then
//   loss2[0] = 12 / (c h w d) * sum,  loss2[1] = lambda * (S_w / N_w + S_h / N_h + S_d / N_d)
struct LossScale {
  double data, reg[3];
};
__global__ __launch_bounds__(256) void instopt_loss_kernel(const float* __restrict__ partial, int nblk, LossScale sc,
                                                           float* __restrict__ loss2) {
  __shared__ double red[256];
  double tot[4];
  for (int q = 0; q < 4; ++q) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) s += (double)partial[(long long)q * nblk + i];
    tot[q] = block_tree_sum<double, 256>(s, red);
  }
  if (threadIdx.x == 0) {
    loss2[0] = (float)(sc.data * tot[0]);
    // diffusion_regularizer adds the w, h, d means in that order (convex_adam_utils.py:97-101)
    loss2[1] = (float)((sc.reg[1] * tot[2] + sc.reg[0] * tot[1]) + sc.reg[2] * tot[3]);
  }
}

// ---- torch.optim.Adam (no weight decay, no amsgrad), the bias corrections formed in double on the host ---------------------
struct AdamStep {
  float w1, b2, w2, step_size, bc2_sqrt, eps;
  int first;            // the moments are zero and are not read (the loop's first update: no launch to clear them)
};
__global__ __launch_bounds__(256) void instopt_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, long long n, AdamStep a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float gi = g[i], m0 = a.first ? 0.f : m[i], v0 = a.first ? 0.f : v[i];
  const float mi = m0 + a.w1 * (gi - m0);                      // lerp(m, g, 1 - beta1), weight < 0.5
  const float vi = v0 * a.b2 + (a.w2 * gi) * gi;
  m[i] = mi;
  v[i] = vi;
  p[i] = p[i] + (-a.step_size * mi) / (sqrtf(vi) / a.bc2_sqrt + a.eps);
}

// ---- the driver's warp ----------------------------------------------------------------------------------------------------
// out[c] = grid_sample(vol[c], identity + (disp / (n - 1) * 2).flip, zeros padding, align_corners=False); one voxel per thread
template <bool NEAREST>
__global__ __launch_bounds__(256) void warp3d_kernel(const float* __restrict__ vol, int C, const float* __restrict__ disp, int H,
                                                     int W, int D, float* __restrict__ out) {
  const long long plane = (long long)H * W * D, o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= plane) return;
  const int x = (int)(o % D), y = (int)((o / D) % W), z = (int)(o / ((long long)D * W));
  const float iz = sample_coord(identity_coord(z, H) + disp[o] / (float)(H - 1) * 2.f, H),
              iy = sample_coord(identity_coord(y, W) + disp[plane + o] / (float)(W - 1) * 2.f, W),
              ix = sample_coord(identity_coord(x, D) + disp[2 * plane + o] / (float)(D - 1) * 2.f, D);
  if (NEAREST) {
    const int zz = (int)rintf(iz), yy = (int)rintf(iy), xx = (int)rintf(ix);      // half to even, as nearbyint
    const bool in = xx >= 0 && xx < D && yy >= 0 && yy < W && zz >= 0 && zz < H;
    const long long p = in ? ((long long)zz * W + yy) * D + xx : 0;
    for (int c = 0; c < C; ++c) out[(long long)c * plane + o] = in ? vol[(long long)c * plane + p] : 0.f;
    return;
  }
  Corners k;
  corners_of(iz, iy, ix, H, W, D, k);
  for (int c = 0; c < C; ++c) {
    const float* src = vol + (long long)c * plane;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += (k.in[j] ? src[k.off[j]] : 0.f) * k.wgt[j];
    out[(long long)c * plane + o] = s;
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
static hipError_t launch_instopt_smooth3(const float* in, float* out, int h, int w, int d, hipStream_t st) {
  const dim3 grid(cdiv(d, kSmX) * cdiv(w, kSmY) * cdiv(h, kSmZ), 3);
  instopt_smooth3_kernel<<<grid, 256, 0, st>>>(in, out, h, w, d);
  return hipGetLastError();
}

static hipError_t launch_sample_grad(const float* ds, const float* fix, const float* mov, int c, int h, int w, int d, float lambda,
                                     float* grad, float* loss2, float* partial, hipStream_t st) {
  const double plane = (double)h * w * d;
  const int n[3] = {h, w, d};
  const double cnt[3] = {3.0 * (h - 1) * w * d, 3.0 * h * (w - 1) * d, 3.0 * h * w * (d - 1)};
  InstoptCoef cf;
  for (int a = 0; a < 3; ++a) {
    cf.half[a] = (float)(n[a] - 1) / 2.f;
    cf.data[a] = (float)(2.0 * 12.0 / ((double)c * plane) * (0.5 * n[a]) / (0.5 * (n[a] - 1)));
    cf.reg[a] = (float)(2.0 * (double)lambda / cnt[a]);
  }
  const int nblk = cdiv((long long)plane, 256);
  if (!loss2) {
    instopt_sample_grad_kernel<false><<<nblk, 256, 0, st>>>(ds, fix, mov, c, h, w, d, cf, grad, nullptr);
    return hipGetLastError();
  }
  instopt_sample_grad_kernel<true><<<nblk, 256, 0, st>>>(ds, fix, mov, c, h, w, d, cf, grad, partial);
  const LossScale sc = {12.0 / ((double)c * plane), {(double)lambda / cnt[0], (double)lambda / cnt[1], (double)lambda / cnt[2]}};
  instopt_loss_kernel<<<1, 256, 0, st>>>(partial, nblk, sc, loss2);
  return hipGetLastError();
}

// scratch of the loop: [disp_sample][grad_sample][grad_weight][exp_avg][exp_avg_sq][loss partials]
struct InstoptLayout {
  size_t ds, gs, gw, m, v, part, total;
};
static InstoptLayout instopt_layout(int h, int w, int d) {
  const size_t plane = (size_t)h * w * d, field = align_up(3 * plane * sizeof(float), 256);
  InstoptLayout L;
  size_t o = 0;
  L.ds = o, o += field;
  L.gs = o, o += field;
  L.gw = o, o += field;
  L.m = o, o += field;
  L.v = o, o += field;
  L.part = o, o += align_up((size_t)4 * cdiv((long long)plane, 256) * sizeof(float), 256);
  L.total = o;
  return L;
}
static size_t instopt_scratch_bytes(int h, int w, int d) { return instopt_layout(h, w, d).total; }

// one iteration's forward and backward from a given weight: smooth, sample + gradient, smooth (3 launches, 4 with the loss)
static hipError_t launch_instopt_grad(const float* weight, const float* fix, const float* mov, int c, int h, int w, int d, float lambda,
                                      float* grad_weight, float* disp_sample, float* loss2, void* scratch, hipStream_t st) {
  const InstoptLayout L = instopt_layout(h, w, d);
  char* base = (char*)scratch;
  float* ds = disp_sample ? disp_sample : (float*)(base + L.ds);
  float* gs = (float*)(base + L.gs);
  hipError_t e = launch_instopt_smooth3(weight, ds, h, w, d, st);
  if (e != hipSuccess) return e;
  e = launch_sample_grad(ds, fix, mov, c, h, w, d, lambda, gs, loss2, (float*)(base + L.part), st);
  if (e != hipSuccess) return e;
  return launch_instopt_smooth3(gs, grad_weight, h, w, d, st);
}

// step t (1-based) of torch.optim.Adam(lr, betas (0.9, 0.999), eps 1e-8): 1 - beta^t, lr / (1 - beta1^t) and sqrt(1 - beta2^t)
// are formed in double, as torch forms them from Python floats, and rounded once
static hipError_t launch_instopt_adam(float* weight, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, double lr, int t,
                                      hipStream_t st, bool zero_moments = false) {
  const double b1 = 0.9, b2 = 0.999;
  const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
  const AdamStep a = {(float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)(lr / bc1), (float)sqrt(bc2), 1e-8f, zero_moments ? 1 : 0};
  instopt_adam_kernel<<<cdiv(n, 256), 256, 0, st>>>(weight, grad, exp_avg, exp_avg_sq, n, a);
  return hipGetLastError();
}

// `niter` iterations; the field returned is the disp_sample of the LAST iteration's forward (weights after niter - 1 updates):
// the reference's last backward and step do not reach its output and are not run.  4 launches per iteration.
static hipError_t launch_instopt(float* weight, const float* fix, const float* mov, int c, int h, int w, int d, float lambda, double lr,
                                 int niter, float* fitted, void* scratch, hipStream_t st) {
  const InstoptLayout L = instopt_layout(h, w, d);
  char* base = (char*)scratch;
  float *gs = (float*)(base + L.gs), *gw = (float*)(base + L.gw), *m = (float*)(base + L.m), *v = (float*)(base + L.v);
  const long long n = 3LL * h * w * d;
  hipError_t e = hipSuccess;
  for (int it = 0; it < niter && e == hipSuccess; ++it) {
    e = launch_instopt_smooth3(weight, fitted, h, w, d, st);
    if (e != hipSuccess || it == niter - 1) break;
    e = launch_sample_grad(fitted, fix, mov, c, h, w, d, lambda, gs, nullptr, nullptr, st);
    if (e == hipSuccess) e = launch_instopt_smooth3(gs, gw, h, w, d, st);
    if (e == hipSuccess) e = launch_instopt_adam(weight, gw, m, v, n, lr, it + 1, st, it == 0);
  }
  return e;
}

// run_instance_opt scratch: [pooled fix][pooled mov][weight][fitted][two full-resolution fields if smoothed][loop scratch]
struct RunLayout {
  size_t pf, pm, wgt, fit, t0, t1, loop, total;
};
static RunLayout run_layout(int c, int H, int W, int D, int g, int smooth) {
  const int h = H / g, w = W / g, d = D / g;
  const size_t plane = (size_t)h * w * d, field = align_up(3 * plane * sizeof(float), 256), feat = align_up((size_t)c * plane * sizeof(float), 256);
  const size_t full = (smooth == 3 || smooth == 5) ? align_up((size_t)3 * H * W * D * sizeof(float), 256) : 0;
  RunLayout L;
  size_t o = 0;
  L.pf = o, o += feat;
  L.pm = o, o += feat;
  L.wgt = o, o += field;
  L.fit = o, o += field;
  L.t0 = o, o += full;
  L.t1 = o, o += full;
  L.loop = o, o += instopt_scratch_bytes(h, w, d);
  L.total = o;
  return L;
}
static size_t run_instopt_scratch_bytes(int c, int H, int W, int D, int g, int smooth) { return run_layout(c, H, W, D, g, smooth).total; }

static hipError_t launch_run_instopt(const float* disp_hr, const float* feat_fix, const float* feat_mov, int c, int H, int W, int D, int g,
                                     float lambda, int niter, int smooth, double lr, float* out, void* scratch, hipStream_t st) {
  const RunLayout L = run_layout(c, H, W, D, g, smooth);
  const int h = H / g, w = W / g, d = D / g;
  char* base = (char*)scratch;
  float *pf = (float*)(base + L.pf), *pm = (float*)(base + L.pm), *wgt = (float*)(base + L.wgt), *fit = (float*)(base + L.fit);
  hipError_t e = launch_pool_cat(nullptr, 0, 1.f, feat_fix, c, 1.f, H, W, D, g, pf, st);
  if (e == hipSuccess) e = launch_pool_cat(nullptr, 0, 1.f, feat_mov, c, 1.f, H, W, D, g, pm, st);
  const float down = (float)(1.0 / (double)g), up = (float)g;
  const float sdown[3] = {down, down, down}, sup[3] = {up, up, up};
  if (e == hipSuccess) e = launch_resize_trilinear(disp_hr, 3, H, W, D, wgt, h, w, d, sdown, 0, st);
  if (e == hipSuccess) e = launch_instopt(wgt, pf, pm, c, h, w, d, lambda, lr, niter, fit, base + L.loop, st);
  if (e != hipSuccess) return e;
  if (smooth != 3 && smooth != 5) return launch_resize_trilinear(fit, 3, h, w, d, out, H, W, D, sup, 0, st);
  float *t0 = (float*)(base + L.t0), *t1 = (float*)(base + L.t1);
  e = launch_resize_trilinear(fit, 3, h, w, d, t0, H, W, D, sup, 0, st);
  if (e == hipSuccess) e = launch_box_filter(t0, t1, 3, H, W, D, smooth, st);
  if (e == hipSuccess) e = launch_box_filter(t1, t0, 3, H, W, D, smooth, st);
  if (e == hipSuccess) e = launch_box_filter(t0, out, 3, H, W, D, smooth, st);
  return e;
}

static hipError_t launch_warp3d(const float* vol, int c, const float* disp, int H, int W, int D, int nearest, float* out, hipStream_t st) {
  const int grid = cdiv((long long)H * W * D, 256);
  if (nearest) warp3d_kernel<true><<<grid, 256, 0, st>>>(vol, c, disp, H, W, D, out);
  else warp3d_kernel<false><<<grid, 256, 0, st>>>(vol, c, disp, H, W, D, out);
  return hipGetLastError();
}

}  // namespace amx

namespace {
using amx::fail;

// the grid of the optimisation: the reference divides by n - 1 and takes means over n - 1 slices
int instopt_grid_check(int c, int h, int w, int d) {
  if (c < 1) return fail(AMX_ERR_INVALID, "c >= 1 (got %d)", c);
  if (h < 2 || w < 2 || d < 2) return fail(AMX_ERR_SHAPE, "the optimisation grid needs at least 2 per axis (got %d, %d, %d)", h, w, d);
  if ((long long)h * w * d >= (1LL << 29)) return fail(AMX_ERR_SHAPE, "grid too large");
  return AMX_OK;
}
bool finite_f(float v) { return v == v && v - v == 0.f; }
}  // namespace

extern "C" {

size_t amx_instance_opt_scratch_bytes(int c, int h, int w, int d) {
  return (c < 1 || h < 2 || w < 2 || d < 2) ? 0 : amx::instopt_scratch_bytes(h, w, d);
}

int amx_instance_opt_smooth3(const float* d_in, float* d_out, int h, int w, int d, void* stream) {
  if (!d_in || !d_out || d_in == d_out) return fail(AMX_ERR_INVALID, "null or aliased argument");
  if (h < 1 || w < 1 || d < 1 || (long long)h * w * d >= (1LL << 29)) return fail(AMX_ERR_SHAPE, "bad shape (%d, %d, %d)", h, w, d);
  AMX_HIP(amx::launch_instopt_smooth3(d_in, d_out, h, w, d, (hipStream_t)stream));
  return AMX_OK;
}

int amx_instance_opt_grad(const float* d_weight, const float* d_fix, const float* d_mov, int c, int h, int w, int d, float lambda,
                          float* d_grad_weight, float* d_disp_sample, float* d_loss2, void* d_scratch, size_t scratch_bytes,
                          void* stream) {
  if (!d_weight || !d_fix || !d_mov || !d_grad_weight || !d_scratch) return fail(AMX_ERR_INVALID, "null argument");
  if (d_grad_weight == d_weight || d_disp_sample == d_weight || d_disp_sample == d_grad_weight)
    return fail(AMX_ERR_INVALID, "outputs must be distinct from the weight and from each other");
  if (int rc = instopt_grid_check(c, h, w, d)) return rc;
  if (!finite_f(lambda)) return fail(AMX_ERR_INVALID, "lambda is not finite");
  if (int rc = amx::need_scratch(amx::instopt_scratch_bytes(h, w, d), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_instopt_grad(d_weight, d_fix, d_mov, c, h, w, d, lambda, d_grad_weight, d_disp_sample, d_loss2, d_scratch,
                                   (hipStream_t)stream));
  return AMX_OK;
}

int amx_instance_opt_adam_step(float* d_weight, const float* d_grad, float* d_exp_avg, float* d_exp_avg_sq, long long n, double lr,
                               int t, void* stream) {
  if (!d_weight || !d_grad || !d_exp_avg || !d_exp_avg_sq) return fail(AMX_ERR_INVALID, "null argument");
  if (n < 1 || n >= (1LL << 31)) return fail(AMX_ERR_SHAPE, "1 <= n < 2^31 (got %lld)", n);
  if (t < 1) return fail(AMX_ERR_INVALID, "step count t >= 1 (got %d)", t);
  if (!(lr > 0.0) || lr - lr != 0.0) return fail(AMX_ERR_INVALID, "lr must be positive and finite");
  AMX_HIP(amx::launch_instopt_adam(d_weight, d_grad, d_exp_avg, d_exp_avg_sq, n, lr, t, (hipStream_t)stream));
  return AMX_OK;
}

int amx_instance_opt(float* d_weight_io, const float* d_fix, const float* d_mov, int c, int h, int w, int d, float lambda, double lr,
                     int niter, float* d_fitted, void* d_scratch, size_t scratch_bytes, void* stream) {
  if (!d_weight_io || !d_fix || !d_mov || !d_fitted || !d_scratch) return fail(AMX_ERR_INVALID, "null argument");
  if (d_fitted == d_weight_io) return fail(AMX_ERR_INVALID, "d_fitted must be distinct from d_weight_io");
  if (int rc = instopt_grid_check(c, h, w, d)) return rc;
  if (niter < 1 || niter > 100000) return fail(AMX_ERR_INVALID, "niter in [1, 100000] (got %d)", niter);
  if (!finite_f(lambda)) return fail(AMX_ERR_INVALID, "lambda is not finite");
  if (!(lr > 0.0) || lr - lr != 0.0) return fail(AMX_ERR_INVALID, "lr must be positive and finite");
  if (int rc = amx::need_scratch(amx::instopt_scratch_bytes(h, w, d), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_instopt(d_weight_io, d_fix, d_mov, c, h, w, d, lambda, lr, niter, d_fitted, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

size_t amx_run_instance_opt_scratch_bytes(int c, int H, int W, int D, int grid_sp_adam, int selected_smooth) {
  if (c < 1 || grid_sp_adam < 1 || H / grid_sp_adam < 2 || W / grid_sp_adam < 2 || D / grid_sp_adam < 2) return 0;
  return amx::run_instopt_scratch_bytes(c, H, W, D, grid_sp_adam, selected_smooth);
}

int amx_run_instance_opt(const float* d_disp_hr, const float* d_feat_fix, const float* d_feat_mov, int c, int H, int W, int D,
                         int grid_sp_adam, float lambda, int niter, int selected_smooth, double lr, float* d_out, void* d_scratch,
                         size_t scratch_bytes, void* stream) {
  if (!d_disp_hr || !d_feat_fix || !d_feat_mov || !d_out || !d_scratch) return fail(AMX_ERR_INVALID, "null argument");
  if (d_out == d_disp_hr) return fail(AMX_ERR_INVALID, "d_out must be distinct from d_disp_hr");
  if (grid_sp_adam < 1) return fail(AMX_ERR_INVALID, "grid_sp_adam >= 1 (got %d)", grid_sp_adam);
  if (H < 1 || W < 1 || D < 1 || (long long)H * W * D >= (1LL << 29)) return fail(AMX_ERR_SHAPE, "bad shape (%d, %d, %d)", H, W, D);
  if (int rc = instopt_grid_check(c, H / grid_sp_adam, W / grid_sp_adam, D / grid_sp_adam)) return rc;
  if (niter < 1 || niter > 100000) return fail(AMX_ERR_INVALID, "niter in [1, 100000] (got %d)", niter);
  if (!finite_f(lambda)) return fail(AMX_ERR_INVALID, "lambda is not finite");
  if (!(lr > 0.0) || lr - lr != 0.0) return fail(AMX_ERR_INVALID, "lr must be positive and finite");
  if (int rc = amx::need_scratch(amx::run_instopt_scratch_bytes(c, H, W, D, grid_sp_adam, selected_smooth), scratch_bytes)) return rc;
  AMX_HIP(amx::launch_run_instopt(d_disp_hr, d_feat_fix, d_feat_mov, c, H, W, D, grid_sp_adam, lambda, niter, selected_smooth, lr,
                                  d_out, d_scratch, (hipStream_t)stream));
  return AMX_OK;
}

int amx_warp3d(const float* d_vol, int c, const float* d_disp, int H, int W, int D, int mode, float* d_out, void* stream) {
  if (!d_vol || !d_disp || !d_out || d_out == d_vol || d_out == d_disp) return fail(AMX_ERR_INVALID, "null or aliased argument");
  if (c < 1) return fail(AMX_ERR_INVALID, "c >= 1 (got %d)", c);
  if (mode != AMX_WARP_BILINEAR && mode != AMX_WARP_NEAREST) return fail(AMX_ERR_INVALID, "mode: AMX_WARP_BILINEAR or AMX_WARP_NEAREST (got %d)", mode);
  if (H < 2 || W < 2 || D < 2 || (long long)H * W * D >= (1LL << 31)) return fail(AMX_ERR_SHAPE, "2 <= extent, volume < 2^31 voxels (got %d, %d, %d)", H, W, D);
  AMX_HIP(amx::launch_warp3d(d_vol, c, d_disp, H, W, D, mode == AMX_WARP_NEAREST, d_out, (hipStream_t)stream));
  return AMX_OK;
}

}  // extern "C"
