// Loss heads of the Cross-Scale MAE step (fp32 reductions, HBM-bound):
//   recon_loss   MAE_ViT_Shared.py:97-163,269-290  patchify-on-the-fly target (+ optional norm_pix), per-patch mse/l2/mae/l1/bce
//   pair_loss    un-masked `.mean()` form used for the cross-decoder (MAE_ViT_MsLdCeCd.py:56-59) and latent (MsLdLe.py:44) terms
//   ntxent       util/contrast_loss.py:44-101 with cos_sim=True, tau=0.5 (mean-pool + normalise fused; masks are analytic)
//   finalize     deterministic single-workgroup reduction of all partial buffers into the scalar terms
//   (the ssim family of recon_loss lives in ssim.hip; what both share, in loss_common.h)
#include "loss_common.h"

// min/max of the processed target per patch (bce's scale_01 works on the whole tensor — MAE_ViT_Shared.py:94-95)
__global__ __launch_bounds__(256) void target_minmax_kernel(PatchGeom g, int norm_pix, long long patches, const float* __restrict__ img0,
                                                            const float* __restrict__ img1, float* __restrict__ mm /*[patches][2]*/) {
  const PatchWave w = patch_wave(g, patches);
  if (!w.live) return;
  const float* img = patch_img(g, img0, img1, w.n2);
  const TargetXform x = target_xform(g, img, w.l, w.lane, norm_pix, LOSS_NONE, nullptr, w.view);
  float lo = INFINITY, hi = -INFINITY;
  for (int e = w.lane; e < g.P; e += 64) { float t = x.apply(patch_elem(g, img, w.l, e)); lo = fminf(lo, t); hi = fmaxf(hi, t); }
  lo = -wave_max(-lo); hi = wave_max(hi);
  if (w.lane == 0) { mm[w.pt * 2] = lo; mm[w.pt * 2 + 1] = hi; }
}
__global__ __launch_bounds__(1024) void minmax_reduce_kernel(long long per_view, int views, const float* __restrict__ mm, float* __restrict__ out /*[views][2]*/) {
  __shared__ float slo[16], shi[16];
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int v = 0; v < views; ++v) {
    float lo = INFINITY, hi = -INFINITY;
    for (long long i = threadIdx.x; i < per_view; i += blockDim.x) { lo = fminf(lo, mm[(v * per_view + i) * 2]); hi = fmaxf(hi, mm[(v * per_view + i) * 2 + 1]); }
    lo = -wave_max(-lo); hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) { slo[w] = lo; shi[w] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) { for (int i = 1; i < nw; ++i) { lo = fminf(lo, slo[i]); hi = fmaxf(hi, shi[i]); } out[v * 2] = lo; out[v * 2 + 1] = hi; }
    __syncthreads();
  }
}

// rowloss[n2*L + l] = mean/sum_e f(pred[n2, 1+l, e], target).  `mask` (nullable): patches with mask 0 are skipped (rowloss 0) — the
// loss only weighs masked patches (MAE_ViT_Shared.py:113-120), three quarters of them at mask_ratio 0.75.
template <typename TP>
__global__ __launch_bounds__(256) void recon_fwd_kernel(PatchGeom g, int kind, int norm_pix, long long patches, const float* __restrict__ img0,
                                                        const float* __restrict__ img1, const TP* __restrict__ pred, long long ldp,
                                                        const float* __restrict__ minmax, const float* __restrict__ mask, float* __restrict__ rowloss) {
  const PatchWave w = patch_wave(g, patches);
  if (!w.live) return;
  if (mask && mask[w.pt] == 0.f) { if (w.lane == 0) rowloss[w.pt] = 0.f; return; }
  const float* img = patch_img(g, img0, img1, w.n2);
  const TargetXform x = target_xform(g, img, w.l, w.lane, norm_pix, kind, minmax, w.view);
  const TP* pr = pred_row(g, pred, ldp, w);
  float s = 0.f;
  for (int e = w.lane; e < g.P; e += 64) s += elem_loss(kind, ld_as_f32<TP>(pr + e), x.apply(patch_elem(g, img, w.l, e)));
  s = wave_sum(s);
  if (w.lane == 0) rowloss[w.pt] = mean_over_last(kind) ? s / g.P : s;
}
// dpred[n2, 1+l, e] = gout * vscale * mask / masksum(view) * f'(pred, t) / (P or 1) (+ extra[n2, l, e], the ssim family's share,
// already scaled, which also reaches visible patches through scale_01's min / max) ; cls rows and pad columns are zeroed
template <typename T, typename TP>
__global__ __launch_bounds__(256) void recon_bwd_kernel(PatchGeom g, int kind, int norm_pix, long long rows, const float* __restrict__ img0,
                                                        const float* __restrict__ img1, const TP* __restrict__ pred, long long ldp,
                                                        const float* __restrict__ minmax, const float* __restrict__ mask,
                                                        const float* __restrict__ losses, const float* __restrict__ gout, float vscale,
                                                        const float* __restrict__ extra, T* __restrict__ dpred, long long ldd) {
  const PatchWave w = patch_row_wave(g, rows);
  if (!w.live) return;
  T* dp = dpred + w.pt * ldd;
  float m = w.l >= 0 ? mask[w.n2 * g.L + w.l] : 0.f;
  const float* ex = (extra && w.l >= 0) ? extra + (w.n2 * g.L + w.l) * g.P : nullptr;
  if (m == 0.f || kind == LOSS_NONE) { for (int e = w.lane; e < ldd; e += 64) st_from_f32<T>(dp + e, (ex && e < g.P) ? ex[e] : 0.f); return; }
  const float* img = patch_img(g, img0, img1, w.n2);
  const TargetXform x = target_xform(g, img, w.l, w.lane, norm_pix, kind, minmax, w.view);
  const float coef = gout[0] * vscale * m / losses[6 + w.view] / (mean_over_last(kind) ? (float)g.P : 1.f);
  const TP* pr = pred + w.pt * ldp;
  for (int e = w.lane; e < ldd; e += 64) {
    float o = 0.f;
    if (e < g.P) {
      o = coef * elem_grad(kind, ld_as_f32<TP>(pr + e), x.apply(patch_elem(g, img, w.l, e)));
      if (ex) o += ex[e];
    }
    st_from_f32<T>(dp + e, o);
  }
}

// ---- throughput forms of the two kernels above for the geometry the step spends its time in: bf16 predictions and bf16 dpred, C * p * p a
// multiple of 128 (ViT-*/16 RGB: P = 768; 4-band: 1024), the mse / l2 / mae / l1 kinds.  A wave owns a patch; a lane owns the element PAIRS
// e = 2 lane + 128 it: the prediction row is read as one 4-byte load per pair (whole 256-byte lines per wave instruction), the 2 NP image
// values of a lane are independent gathers that are all in flight before the first use (the generic form walks the patch with a runtime
// trip count: one dependent load pair per iteration), and the image is read ONCE also under norm_pix_loss (the values stay in registers
// for the statistics).  Same per-element arithmetic as the generic kernels (the partial sums are taken in another order).
template <int C, int P_, int NP>
__device__ __forceinline__ void patch_load_pairs(const PatchGeom& g, const float* __restrict__ img, int l, int lane, float (&t)[2 * NP]) {
  const int gh = l / g.G, gw = l - gh * g.G;
  const float* base = img + ((long long)gh * P_) * g.S + gw * P_;
#pragma unroll
  for (int it = 0; it < NP; ++it)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = 2 * lane + 128 * it + k, r = e / C, c = e - r * C, ph = r / P_, pw = r - ph * P_;
      t[2 * it + k] = base[((long long)c * g.S + ph) * g.S + pw];
    }
}
template <int NV>
__device__ __forceinline__ void patch_normalise(int P, float (&t)[NV]) {   // norm_pix_loss: unbiased variance, eps 1e-6
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) s += t[k];
  const float mu = wave_sum(s) / P;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) { const float d = t[k] - mu; q += d * d; }
  const TargetXform x{mu, rsqrtf(wave_sum(q) / (P - 1) + 1.0e-6f), 0.f, 1.f, false};
#pragma unroll
  for (int k = 0; k < NV; ++k) t[k] = x.apply(t[k]);
}
template <int C, int P_, int NP>
__global__ __launch_bounds__(256) void recon_fwd_fast_kernel(PatchGeom g, int kind, int norm_pix, long long patches, const float* __restrict__ img0,
                                                             const float* __restrict__ img1, const bf16_t* __restrict__ pred, long long ldp,
                                                             const float* __restrict__ mask, float* __restrict__ rowloss) {
  const PatchWave w = patch_wave(g, patches);
  if (!w.live) return;
  if (mask && mask[w.pt] == 0.f) { if (w.lane == 0) rowloss[w.pt] = 0.f; return; }
  const unsigned* pr = reinterpret_cast<const unsigned*>(pred_row(g, pred, ldp, w)) + w.lane;
  unsigned pv[NP];
#pragma unroll
  for (int it = 0; it < NP; ++it) pv[it] = pr[64 * it];
  float t[2 * NP];
  patch_load_pairs<C, P_, NP>(g, patch_img(g, img0, img1, w.n2), w.l, w.lane, t);
  if (norm_pix) patch_normalise<2 * NP>(g.P, t);
  float s = 0.f;
#pragma unroll
  for (int it = 0; it < NP; ++it) {
    s += elem_loss(kind, __uint_as_float(pv[it] << 16), t[2 * it]);
    s += elem_loss(kind, __uint_as_float(pv[it] & 0xffff0000u), t[2 * it + 1]);
  }
  s = wave_sum(s);
  if (w.lane == 0) rowloss[w.pt] = mean_over_last(kind) ? s / g.P : s;
}
template <int C, int P_, int NP>
__global__ __launch_bounds__(256) void recon_bwd_fast_kernel(PatchGeom g, int kind, int norm_pix, long long rows, const float* __restrict__ img0,
                                                             const float* __restrict__ img1, const bf16_t* __restrict__ pred, long long ldp,
                                                             const float* __restrict__ mask, const float* __restrict__ losses,
                                                             const float* __restrict__ gout, float vscale, bf16_t* __restrict__ dpred, long long ldd) {
  const PatchWave w = patch_row_wave(g, rows);
  if (!w.live) return;
  unsigned* dp = reinterpret_cast<unsigned*>(dpred + w.pt * ldd) + w.lane;   // (ldd == P here: no pad columns)
  const float m = w.l >= 0 ? mask[w.n2 * g.L + w.l] : 0.f;
  if (m == 0.f) {
#pragma unroll
    for (int it = 0; it < NP; ++it) dp[64 * it] = 0u;
    return;
  }
  const unsigned* pr = reinterpret_cast<const unsigned*>(pred + w.pt * ldp) + w.lane;
  unsigned pv[NP];
#pragma unroll
  for (int it = 0; it < NP; ++it) pv[it] = pr[64 * it];
  float t[2 * NP];
  patch_load_pairs<C, P_, NP>(g, patch_img(g, img0, img1, w.n2), w.l, w.lane, t);
  if (norm_pix) patch_normalise<2 * NP>(g.P, t);
  const float coef = gout[0] * vscale * m / losses[6 + w.view] / (mean_over_last(kind) ? (float)g.P : 1.f);
#pragma unroll
  for (int it = 0; it < NP; ++it)
    dp[64 * it] = pack2bf(coef * elem_grad(kind, __uint_as_float(pv[it] << 16), t[2 * it]), coef * elem_grad(kind, __uint_as_float(pv[it] & 0xffff0000u), t[2 * it + 1]));
}
static bool recon_fast_geometry(int kind, int C, int p, long long ldp, long long ldd) {
  return kind >= LOSS_MSE && kind <= LOSS_L1 && p == 16 && (C == 3 || C == 4) && ldp % 2 == 0 && ldd == (long long)C * p * p;
}

// the two geometries of the fast kernels: RGB (P = 768, 6 element pairs per lane) and 4-band (P = 1024, 8)
#define RECON_FAST_KERNEL(K, C) ((C) == 3 ? K<3, 16, 6> : K<4, 16, 8>)

void loss_launch_target_minmax(const PatchGeom& g, int norm_pix, long long patches, const float* img0, const float* img1, float* mm, hipStream_t st) {
  hipLaunchKernelGGL(target_minmax_kernel, dim3(cdiv(patches, 4)), dim3(256), 0, st, g, norm_pix, patches, img0, img1, mm);
}
void loss_launch_minmax_reduce(long long per_view, int views, const float* mm, float* out, hipStream_t st) {
  hipLaunchKernelGGL(minmax_reduce_kernel, dim3(1), dim3(1024), 0, st, per_view, views, mm, out);
}
extern "C" int csmae_target_minmax(int norm_pix, long long B2, int N, int C, int S, int p, const float* img0, const float* img1,
                                   float* scratch /*[B2*L*2]*/, float* out /*[views*2]*/, void* stream) {
  PatchGeom g = make_geom(N, C, S, p);
  loss_launch_target_minmax(g, norm_pix, B2 * g.L, img0, img1, scratch, (hipStream_t)stream);
  loss_launch_minmax_reduce((long long)N * g.L, (int)(B2 / N), scratch, out, (hipStream_t)stream);
  return csmae_check_launch("csmae_target_minmax");
}
extern "C" int csmae_recon_loss_fwd(int kind, int norm_pix, int pred_dtype, long long B2, int N, int C, int S, int p, const float* img0, const float* img1,
                                    const void* pred, long long ldp, const float* minmax, const float* mask, float* rowloss, void* stream) {
  CSMAE_REQUIRE(kind >= LOSS_MSE && kind <= LOSS_BCE, "csmae_recon_loss_fwd: loss kind %d is outside the hot-path scope (ssim family: SURVEY §2 row 2)", kind);
  CSMAE_REQUIRE(B2 > 0 && N > 0 && B2 % N == 0 && S % p == 0 && (kind != LOSS_BCE || minmax), "csmae_recon_loss_fwd: bad args");
  CSMAE_REQUIRE(pred_dtype == CSMAE_F32 || pred_dtype == CSMAE_BF16, "csmae_recon_loss_fwd: bad prediction dtype %d", pred_dtype);
  PatchGeom g = make_geom(N, C, S, p);
  long long patches = B2 * g.L;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(cdiv(patches, 4)), block(256);
  if (pred_dtype == CSMAE_BF16 && recon_fast_geometry(kind, C, p, ldp, g.P))
    hipLaunchKernelGGL(RECON_FAST_KERNEL(recon_fwd_fast_kernel, C), grid, block, 0, st, g, kind, norm_pix, patches, img0, img1, (const bf16_t*)pred, ldp, mask, rowloss);
  else if (pred_dtype == CSMAE_BF16) hipLaunchKernelGGL((recon_fwd_kernel<bf16_t>), grid, block, 0, st, g, kind, norm_pix, patches, img0, img1, (const bf16_t*)pred, ldp, minmax, mask, rowloss);
  else hipLaunchKernelGGL((recon_fwd_kernel<float>), grid, block, 0, st, g, kind, norm_pix, patches, img0, img1, (const float*)pred, ldp, minmax, mask, rowloss);
  return csmae_check_launch("csmae_recon_loss_fwd");
}
extern "C" int csmae_recon_loss_bwd(int kind, int norm_pix, int out_dtype, int pred_dtype, long long B2, int N, int C, int S, int p, const float* img0,
                                    const float* img1, const void* pred, long long ldp, const float* minmax, const float* mask,
                                    const float* losses, const float* gout, float vscale, const float* extra, void* dpred, long long ldd,
                                    void* stream) {
  CSMAE_REQUIRE(kind >= LOSS_MSE && kind <= LOSS_NONE && (kind != LOSS_NONE || extra), "csmae_recon_loss_bwd: bad loss kind %d", kind);
  CSMAE_REQUIRE((out_dtype == CSMAE_F32 || out_dtype == CSMAE_BF16) && (pred_dtype == CSMAE_F32 || pred_dtype == CSMAE_BF16), "csmae_recon_loss_bwd: bad dtype %d / %d", out_dtype, pred_dtype);
  PatchGeom g = make_geom(N, C, S, p);
  long long rows = B2 * (g.L + 1);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(cdiv(rows, 4)), block(256);
#define RECON_BWD(T, TP) hipLaunchKernelGGL((recon_bwd_kernel<T, TP>), grid, block, 0, st, g, kind, norm_pix, rows, img0, img1, (const TP*)pred, ldp, minmax, mask, losses, gout, vscale, extra, (T*)dpred, ldd)
  if (out_dtype == CSMAE_BF16 && pred_dtype == CSMAE_BF16 && !extra && recon_fast_geometry(kind, C, p, ldp, ldd))
    hipLaunchKernelGGL(RECON_FAST_KERNEL(recon_bwd_fast_kernel, C), grid, block, 0, st, g, kind, norm_pix, rows, img0, img1, (const bf16_t*)pred, ldp, mask, losses, gout, vscale, (bf16_t*)dpred, ldd);
  else if (out_dtype == CSMAE_BF16 && pred_dtype == CSMAE_BF16) RECON_BWD(bf16_t, bf16_t);
  else if (out_dtype == CSMAE_BF16) RECON_BWD(bf16_t, float);
  else if (pred_dtype == CSMAE_BF16) RECON_BWD(float, bf16_t);
  else RECON_BWD(float, float);
#undef RECON_BWD
  return csmae_check_launch("csmae_recon_loss_bwd");
}

// ------------------------------------------------------------------------------------------ un-masked pair loss
// view row r -> storage row (r / group) * gstride + off + r % group  (same convention as rows_gather)
struct RowView { long long group, gstride, off; };
__device__ __forceinline__ long long vrow(const RowView& v, long long r) { return (r / v.group) * v.gstride + v.off + r % v.group; }
#define PAIR_BLOCKS 512
__global__ __launch_bounds__(256) void pair_fwd_kernel(int kind, long long rows, int D, const float* __restrict__ a, RowView va,
                                                       const float* __restrict__ t, RowView vt, float* __restrict__ partial) {
  __shared__ float red[32];
  const int dv = D >> 2;
  float s = 0.f;
  // items = (row, 16-byte column) pairs, grid-strided: every thread has work whatever the row length (a 512-wide row is 128 items: half of a
  // workgroup idled when a workgroup walked one row at a time), two items per trip so that four loads are in flight
  const long long items = rows * dv, step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += 2 * step) {
    const long long r0 = i / dv, i1 = i + step;
    const int c0 = (int)(i - r0 * dv);
    f4_t x0 = *reinterpret_cast<const f4_t*>(a + vrow(va, r0) * D + c0 * 4), y0 = *reinterpret_cast<const f4_t*>(t + vrow(vt, r0) * D + c0 * 4);
    if (i1 < items) {
      const long long r1 = i1 / dv; const int c1 = (int)(i1 - r1 * dv);
      f4_t x1 = *reinterpret_cast<const f4_t*>(a + vrow(va, r1) * D + c1 * 4), y1 = *reinterpret_cast<const f4_t*>(t + vrow(vt, r1) * D + c1 * 4);
      for (int k = 0; k < 4; ++k) s += elem_loss(kind, x1[k], y1[k]);
    }
    for (int k = 0; k < 4; ++k) s += elem_loss(kind, x0[k], y0[k]);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// d/da = gout * coef * f'(a - t); d/dt = -that.  da_lp: low-precision copy (GEMM operand); *_acc: fp32 += into residual-grad buffers
template <typename T>
__global__ __launch_bounds__(256) void pair_bwd_kernel(int kind, long long rows, int D, const float* __restrict__ a, RowView va,
                                                       const float* __restrict__ t, RowView vt, const float* __restrict__ gout, float coef,
                                                       T* __restrict__ da_lp, float* __restrict__ da_acc, float* __restrict__ dt_acc) {
  const int dv = D >> 2;
  const float cf = gout[0] * coef;
  for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
    const long long ra = vrow(va, r), rt = vrow(vt, r);
    for (int c = threadIdx.x; c < dv; c += blockDim.x) {
      f4_t x = *reinterpret_cast<const f4_t*>(a + ra * D + c * 4), y = *reinterpret_cast<const f4_t*>(t + rt * D + c * 4), g;
      for (int k = 0; k < 4; ++k) g[k] = cf * elem_grad(kind, x[k], y[k]);
      if (da_lp) st4<T>(da_lp + r * D + c * 4, g);
      if (da_acc) { f4_t o = *reinterpret_cast<f4_t*>(da_acc + ra * D + c * 4) + g; *reinterpret_cast<f4_t*>(da_acc + ra * D + c * 4) = o; }
      if (dt_acc) { f4_t o = *reinterpret_cast<f4_t*>(dt_acc + rt * D + c * 4) - g; *reinterpret_cast<f4_t*>(dt_acc + rt * D + c * 4) = o; }
    }
  }
}
extern "C" int csmae_pair_loss_fwd(int kind, long long rows, int D, const float* a, long long a_group, long long a_gstride, long long a_off,
                                   const float* t, long long t_group, long long t_gstride, long long t_off, float* partial /*[512]*/, void* stream) {
  CSMAE_REQUIRE(kind >= LOSS_MSE && kind <= LOSS_L1, "csmae_pair_loss: kind %d unsupported for un-masked pair losses (mse/l2/mae/l1 only)", kind);
  CSMAE_REQUIRE(rows > 0 && D % 4 == 0, "csmae_pair_loss_fwd: bad geometry");
  RowView va{a_group, a_gstride, a_off}, vt{t_group, t_gstride, t_off};
  hipLaunchKernelGGL(pair_fwd_kernel, dim3(PAIR_BLOCKS), dim3(256), 0, (hipStream_t)stream, kind, rows, D, a, va, t, vt, partial);
  return csmae_check_launch("csmae_pair_loss_fwd");
}
extern "C" int csmae_pair_loss_bwd(int kind, int lp_dtype, long long rows, int D, const float* a, long long a_group, long long a_gstride, long long a_off,
                                   const float* t, long long t_group, long long t_gstride, long long t_off, const float* gout, float coef,
                                   void* da_lp, float* da_acc, float* dt_acc, void* stream) {
  CSMAE_REQUIRE(kind >= LOSS_MSE && kind <= LOSS_L1, "csmae_pair_loss: kind %d unsupported for un-masked pair losses (mse/l2/mae/l1 only)", kind);
  RowView va{a_group, a_gstride, a_off}, vt{t_group, t_gstride, t_off};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(rows < 8192 ? rows : 8192));   // (2 048 workgroups walked 12 rows each one after the other: 1.5-2.5 TB/s; every CU's share resident at once)
  if (lp_dtype == CSMAE_BF16) hipLaunchKernelGGL((pair_bwd_kernel<bf16_t>), grid, dim3(128), 0, st, kind, rows, D, a, va, t, vt, gout, coef, (bf16_t*)da_lp, da_acc, dt_acc);
  else hipLaunchKernelGGL((pair_bwd_kernel<float>), grid, dim3(128), 0, st, kind, rows, D, a, va, t, vt, gout, coef, (float*)da_lp, da_acc, dt_acc);
  return csmae_check_launch("csmae_pair_loss_bwd");
}

// ------------------------------------------------------------------------------------------ NT-Xent (cosine, per-GPU negatives)
// z_i = normalize(mean_t latent[i, 1+t, :]);  e_ij = exp(z_i.z_j / tau);  pos_i = e_{i, i+-N};  neg_i = sum_{j != i, j != partner} e_ij
// rowloss_i = -log(pos_i / (neg_i + eps))        (positives are NOT in the denominator — contrast_loss.py:28,94-99)
__global__ __launch_bounds__(256) void ntx_pool_kernel(int Te, int keep, int D, const float* __restrict__ latent, float* __restrict__ z, float* __restrict__ inv_norm) {
  __shared__ float red[32];
  const long long i = blockIdx.x;
  float q = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float s = 0.f;
    for (int t = 0; t < keep; ++t) s += latent[(i * Te + 1 + t) * D + d];
    s /= keep;
    z[i * D + d] = s; q += s * s;
  }
  q = block_sum(q, red);
  const float inv = 1.f / fmaxf(sqrtf(q), 1e-12f);
  for (int d = threadIdx.x; d < D; d += blockDim.x) z[i * D + d] *= inv;
  if (threadIdx.x == 0) inv_norm[i] = inv;
}
// The grouped column fold of ntx_pool4_kernel and ntx_bwd4_kernel: G groups of D / 4 threads, thread (g, c) sums the 16-byte column c of the rows
// g, g + G, ... of `base` (WEIGHTED: times coef[row]) with four loads in flight, then group 0 folds the groups' sums through part[] in group order
template <bool WEIGHTED>
__device__ __forceinline__ f4_t ntx_group_fold(const float* __restrict__ base, int rows, int D, int G, int g, int c, const float* coef, f4_t* part /*[1024]*/) {
  f4_t s = {0.f, 0.f, 0.f, 0.f};
  if (g < G) {
    auto row = [&](int j) { return *reinterpret_cast<const f4_t*>(base + (long long)j * D + c * 4); };
    int j = g;
    for (; j + 3 * G < rows; j += 4 * G) {
      const f4_t a0 = row(j), a1 = row(j + G), a2 = row(j + 2 * G), a3 = row(j + 3 * G);
      if (WEIGHTED) s += (a0 * coef[j] + a1 * coef[j + G]) + (a2 * coef[j + 2 * G] + a3 * coef[j + 3 * G]);
      else s += (a0 + a1) + (a2 + a3);
    }
    for (; j < rows; j += G) { if (WEIGHTED) s += row(j) * coef[j]; else s += row(j); }
    part[threadIdx.x] = s;
  }
  __syncthreads();
  if (g == 0) for (int k = 1; k < G; ++k) s += part[k * (D >> 2) + c];
  return s;
}
// The same for D % 4 == 0, D <= 4096 (every geometry of the step): the sample's keep x D values are walked by ALL 1024 threads — G = 1024 / (D / 4)
// groups of rows, a thread owns one 16-byte column of every G-th row, its loads independent of each other — and folded through LDS in group
// order (deterministic).  The first form gave a thread a whole column: `keep` dependent 4-byte loads, 256 threads per sample (0.65 TB/s).
__global__ __launch_bounds__(1024) void ntx_pool4_kernel(int Te, int keep, int D, const float* __restrict__ latent, float* __restrict__ z, float* __restrict__ inv_norm) {
  __shared__ float red[32];
  __shared__ f4_t part[1024];
  const long long i = blockIdx.x;
  const int dv = D >> 2, G = 1024 / dv, g = threadIdx.x / dv, c = threadIdx.x - g * dv;
  f4_t s = ntx_group_fold<false>(latent + (i * Te + 1) * D, keep, D, G, g, c, nullptr, part);
  float q = 0.f;
  if (g == 0) {
    s = s / (float)keep;
    q = s[0] * s[0] + s[1] * s[1] + s[2] * s[2] + s[3] * s[3];
  }
  q = block_sum(q, red);
  const float inv = 1.f / fmaxf(sqrtf(q), 1e-12f);
  if (g == 0) *reinterpret_cast<f4_t*>(z + i * D + c * 4) = s * inv;
  if (threadIdx.x == 0) inv_norm[i] = inv;
}
__global__ __launch_bounds__(1024) void ntx_sim_kernel(int N, int D, const float* __restrict__ z, float tau, float eps, float* __restrict__ E,
                                                      float* __restrict__ neg, float* __restrict__ rowloss) {
  __shared__ float red[32];
  extern __shared__ float zi[];
  const int i = blockIdx.x, B2 = 2 * N, partner = (i + N) % B2;
  for (int d = threadIdx.x; d < D; d += blockDim.x) zi[d] = z[(long long)i * D + d];
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool vec = (D & 3) == 0;
  float nsum = 0.f;
  for (int j0 = 4 * w; j0 < B2; j0 += 4 * (blockDim.x >> 6)) {  // four rows per wave iteration: independent load chains, one pass over z_i
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {   // 16-byte loads: D / 256 trips with four rows' loads in flight (scalar loads made this a 12-trip dependent walk at D = 768)
      for (int d = lane * 4; d < D; d += 256) {
        const f4_t a = *reinterpret_cast<const f4_t*>(zi + d);
#pragma unroll
        for (int u = 0; u < 4; ++u) if (j0 + u < B2) {
          const f4_t b = *reinterpret_cast<const f4_t*>(z + (long long)(j0 + u) * D + d);
          s[u] += (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
        }
      }
    } else {
      for (int d = lane; d < D; d += 64) {
        const float a = zi[d];
#pragma unroll
        for (int u = 0; u < 4; ++u) if (j0 + u < B2) s[u] += a * z[(long long)(j0 + u) * D + d];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u;
      const float e = expf(wave_sum(s[u]) / tau);
      if (lane == 0 && j < B2) { E[(long long)i * B2 + j] = e; if (j != i && j != partner) nsum += e; }
    }
  }
  nsum = block_sum(nsum, red);
  if (threadIdx.x == 0) neg[i] = nsum;
  __syncthreads();
  if (threadIdx.x == 0) rowloss[i] = -logf(E[(long long)i * B2 + partner] / (nsum + eps));
}
// dL/dc_ij = w * ( [j neg] e_ij / (tau (neg_i+eps))  -  [j == partner] / tau ),  w = gout / 2N ;  dz_i = sum_j (G_ij + G_ji) z_j
// then through F.normalize: df = (dz - z (z.dz)) * inv_norm ; dpool = df (the 1/keep of the mean is applied by latent_grad_finish)
__device__ __forceinline__ void ntx_coef_fill(float* coef /*[2N], LDS*/, int i, int N, const float* __restrict__ E, const float* __restrict__ neg, float tau, float eps, float w) {
  const int B2 = 2 * N, partner = (i + N) % B2;
  for (int j = threadIdx.x; j < B2; j += blockDim.x) {
    float c = 0.f;
    if (j == partner) c = -2.f * w / tau;  // G_ip + G_pi
    else if (j != i) c = w / tau * (E[(long long)i * B2 + j] / (neg[i] + eps) + E[(long long)j * B2 + i] / (neg[j] + eps));
    coef[j] = c;
  }
  __syncthreads();
}
__global__ __launch_bounds__(1024) void ntx_bwd_kernel(int N, int D, const float* __restrict__ z, const float* __restrict__ inv_norm,
                                                      const float* __restrict__ E, const float* __restrict__ neg, float tau, float eps,
                                                      const float* __restrict__ gout, float* __restrict__ dpool) {
  __shared__ float red[32];
  extern __shared__ float coef[];  // [2N]
  const int i = blockIdx.x, B2 = 2 * N;
  ntx_coef_fill(coef, i, N, E, neg, tau, eps, gout[0] / B2);
  float dot = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float s = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;   // four independent chains: the 2N-long walk is latency-, not bandwidth-bound
    int j = 0;
    for (; j + 3 < B2; j += 4) {
      s += coef[j] * z[(long long)j * D + d]; s1 += coef[j + 1] * z[(long long)(j + 1) * D + d];
      s2 += coef[j + 2] * z[(long long)(j + 2) * D + d]; s3 += coef[j + 3] * z[(long long)(j + 3) * D + d];
    }
    for (; j < B2; ++j) s += coef[j] * z[(long long)j * D + d];
    s = (s + s1) + (s2 + s3);
    dpool[(long long)i * D + d] = s;
    dot += s * z[(long long)i * D + d];
  }
  dot = block_sum(dot, red);
  const float inv = inv_norm[i];
  for (int d = threadIdx.x; d < D; d += blockDim.x) dpool[(long long)i * D + d] = (dpool[(long long)i * D + d] - z[(long long)i * D + d] * dot) * inv;
}
// The same for D % 4 == 0, D <= 4096: 16-byte columns, the 2N-long walk split over G = 1024 / (D / 4) groups of threads with four loads in flight
// each, folded through LDS in group order (the first form: one 4-byte column per thread, 2N dependent-latency trips; it sits on the main
// chain between the decoder's and the encoder's backward).
__global__ __launch_bounds__(1024) void ntx_bwd4_kernel(int N, int D, const float* __restrict__ z, const float* __restrict__ inv_norm,
                                                       const float* __restrict__ E, const float* __restrict__ neg, float tau, float eps,
                                                       const float* __restrict__ gout, float* __restrict__ dpool) {
  __shared__ float red[32];
  __shared__ f4_t part[1024];
  extern __shared__ float coef[];  // [2N]
  const int i = blockIdx.x, B2 = 2 * N;
  ntx_coef_fill(coef, i, N, E, neg, tau, eps, gout[0] / B2);
  const int dv = D >> 2, G = 1024 / dv, g = threadIdx.x / dv, c = threadIdx.x - g * dv;
  f4_t s = ntx_group_fold<true>(z, B2, D, G, g, c, coef, part);
  float dot = 0.f;
  f4_t zi = {0.f, 0.f, 0.f, 0.f};
  if (g == 0) {
    zi = *reinterpret_cast<const f4_t*>(z + (long long)i * D + c * 4);
    dot = (s[0] * zi[0] + s[1] * zi[1]) + (s[2] * zi[2] + s[3] * zi[3]);
  }
  dot = block_sum(dot, red);
  if (g == 0) *reinterpret_cast<f4_t*>(dpool + (long long)i * D + c * 4) = (s - zi * dot) * inv_norm[i];
}
extern "C" int csmae_ntxent_fwd(int N, int Te, int keep, int D, const float* latent, float tau, float eps, float* z, float* inv_norm,
                                float* E, float* neg, float* rowloss, void* stream) {
  CSMAE_REQUIRE(N > 0 && keep > 0 && keep < Te && D > 0 && D * 4 <= 64 * 1024, "csmae_ntxent_fwd: bad geometry N=%d Te=%d keep=%d D=%d", N, Te, keep, D);
  hipStream_t st = (hipStream_t)stream;
  if (D % 4 == 0 && D <= 4096) hipLaunchKernelGGL(ntx_pool4_kernel, dim3(2 * N), dim3(1024), 0, st, Te, keep, D, latent, z, inv_norm);
  else hipLaunchKernelGGL(ntx_pool_kernel, dim3(2 * N), dim3(256), 0, st, Te, keep, D, latent, z, inv_norm);
  hipLaunchKernelGGL(ntx_sim_kernel, dim3(2 * N), dim3(1024), D * sizeof(float), st, N, D, z, tau, eps, E, neg, rowloss);
  return csmae_check_launch("csmae_ntxent_fwd");
}
extern "C" int csmae_ntxent_bwd(int N, int D, const float* z, const float* inv_norm, const float* E, const float* neg, float tau, float eps,
                                const float* gout, float* dpool, void* stream) {
  CSMAE_REQUIRE(N > 0 && D > 0 && 2 * N * 4 <= 64 * 1024, "csmae_ntxent_bwd: bad geometry");
  if (D % 4 == 0 && D <= 4096) hipLaunchKernelGGL(ntx_bwd4_kernel, dim3(2 * N), dim3(1024), 2 * N * sizeof(float), (hipStream_t)stream, N, D, z, inv_norm, E, neg, tau, eps, gout, dpool);
  else hipLaunchKernelGGL(ntx_bwd_kernel, dim3(2 * N), dim3(D >= 1024 ? 1024 : ((D + 63) / 64) * 64), 2 * N * sizeof(float), (hipStream_t)stream, N, D, z, inv_norm, E, neg, tau, eps, gout, dpool);
  return csmae_check_launch("csmae_ntxent_bwd");
}
// dlat[n, t>=1, :] += dpool[n, :] * inv_keep ; then emit the low-precision copy that the encoder backward GEMMs consume
template <typename T>
__global__ __launch_bounds__(256) void latent_grad_finish_kernel(long long rows, int Te, int D, float* __restrict__ dlat, const float* __restrict__ dpool,
                                                                 float inv_keep, T* __restrict__ dlat_lp) {
  const int dv = D >> 2;
  for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
    const long long n = r / Te; const int t = (int)(r - n * Te);
    for (int c = threadIdx.x; c < dv; c += blockDim.x) {
      f4_t g = *reinterpret_cast<f4_t*>(dlat + r * D + c * 4);
      if (dpool && t > 0) { g += *reinterpret_cast<const f4_t*>(dpool + n * D + c * 4) * inv_keep; *reinterpret_cast<f4_t*>(dlat + r * D + c * 4) = g; }
      if (dlat_lp) st4<T>(dlat_lp + r * D + c * 4, g);
    }
  }
}
extern "C" int csmae_latent_grad_finish(int lp_dtype, long long B2, int Te, int D, float* dlat, const float* dpool, float inv_keep, void* dlat_lp, void* stream) {
  CSMAE_REQUIRE(B2 > 0 && Te > 0 && D % 4 == 0, "csmae_latent_grad_finish: bad geometry");
  long long rows = B2 * Te;
  dim3 grid((unsigned)fmin((double)rows, 4096.0)), block(D >= 1024 ? 256 : 128);
  hipStream_t st = (hipStream_t)stream;
  if (lp_dtype == CSMAE_BF16) hipLaunchKernelGGL((latent_grad_finish_kernel<bf16_t>), grid, block, 0, st, rows, Te, D, dlat, dpool, inv_keep, (bf16_t*)dlat_lp);
  else hipLaunchKernelGGL((latent_grad_finish_kernel<float>), grid, block, 0, st, rows, Te, D, dlat, dpool, inv_keep, (float*)dlat_lp);
  return csmae_check_launch("csmae_latent_grad_finish");
}

// ------------------------------------------------------------------------------------------ scalar assembly
// losses[0]=total [1]=recon orig [2]=recon crop [3]=cross-decoder [4]=contrastive [5]=latent [6]=sum(mask) orig [7]=sum(mask) crop
// One pass over everything with independent accumulators and 16-byte loads, ONE seven-value block reduction (the first form walked the two
// views one after the other with a dependent scalar chain each and ran seven block reductions of three barriers: 29 us on the critical path
// between forward and backward).  Fixed thread-to-element assignment and fold order: deterministic.
__global__ __launch_bounds__(1024) void finalize_kernel(long long per_view, int views, const float* __restrict__ rowloss, const float* __restrict__ mask,
                                                       float recon_scale, const float* __restrict__ cd_partial, float cd_scale,
                                                       const float* __restrict__ e_partial, float e_scale, const float* __restrict__ ce_rowloss,
                                                       int ce_rows, float* __restrict__ losses) {
  __shared__ float red[16][8];
  float v[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // num0, den0, num1, den1, cd, e, ce
  const long long total = per_view * views;
  if ((per_view & 3) == 0) {
    for (long long i = (long long)threadIdx.x * 4; i < total; i += 4096) {
      const f4_t r = *reinterpret_cast<const f4_t*>(rowloss + i), m = *reinterpret_cast<const f4_t*>(mask + i);
      const float num = (r[0] * m[0] + r[1] * m[1]) + (r[2] * m[2] + r[3] * m[3]), den = (m[0] + m[1]) + (m[2] + m[3]);
      if (i < per_view) { v[0] += num; v[1] += den; } else { v[2] += num; v[3] += den; }
    }
  } else {
    for (long long i = threadIdx.x; i < total; i += 1024) {
      const float m = mask[i], num = rowloss[i] * m;
      if (i < per_view) { v[0] += num; v[1] += m; } else { v[2] += num; v[3] += m; }
    }
  }
  if (cd_partial) for (int i = threadIdx.x; i < PAIR_BLOCKS; i += 1024) v[4] += cd_partial[i];
  if (e_partial) for (int i = threadIdx.x; i < PAIR_BLOCKS; i += 1024) v[5] += e_partial[i];
  if (ce_rowloss) for (int i = threadIdx.x; i < ce_rows; i += 1024) v[6] += ce_rowloss[i];
#pragma unroll
  for (int k = 0; k < 7; ++k) v[k] = wave_sum(v[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k) red[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t[7];
    for (int k = 0; k < 7; ++k) { float a = 0.f; for (int w = 0; w < 16; ++w) a += red[w][k]; t[k] = a; }
    const float l0 = t[0] / t[1];                              // mask_ratio = 0 -> 0/0 = NaN, as in the reference (MAE_ViT_Shared.py:119)
    const float l1 = views > 1 ? t[2] / t[3] : 0.f;
    const float cd = cd_partial ? t[4] * cd_scale : 0.f, e = e_partial ? t[5] * e_scale : 0.f, ce = ce_rowloss ? t[6] / ce_rows : 0.f;
    losses[1] = l0; losses[2] = l1; losses[6] = t[1]; losses[7] = views > 1 ? t[3] : 0.f;
    losses[3] = cd; losses[4] = ce; losses[5] = e;
    losses[0] = (l0 * recon_scale + l1 * recon_scale) + cd + ce + e;
  }
}
extern "C" int csmae_loss_finalize(long long per_view, int views, const float* rowloss, const float* mask, float recon_scale,
                                   const float* cd_partial, float cd_scale, const float* e_partial, float e_scale,
                                   const float* ce_rowloss, int ce_rows, float* losses, void* stream) {
  CSMAE_REQUIRE(per_view > 0 && (views == 1 || views == 2) && losses, "csmae_loss_finalize: bad args");
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, per_view, views, rowloss, mask, recon_scale, cd_partial, cd_scale, e_partial, e_scale, ce_rowloss, ce_rows, losses);
  return csmae_check_launch("csmae_loss_finalize");
}
