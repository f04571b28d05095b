// The ssim family of the reconstruction loss: ssim, ms_ssim and their mse_* mixtures.
// MAE_ViT_Shared.py:165-267 around pytorch-msssim 0.2.1 (`env.yml:118`): both operands are min-max scaled over the whole per-view
// tensor (scale_01 :94-95), un-patchified, multiplied by the patch mask, then compared with ssim(data_range 1, nonnegative) or the
// five-scale ms_ssim.  HBM-bound stencils: planes [B2*C][H][W] fp32 per level, an 11-tap separable gaussian ("valid" windows, the
// H axis first as the package does), 32x32 tiles staged through LDS.  All reductions are two-stage and deterministic.
//   workspace (floats): see SsimLayout.  X = prediction planes, Y = target planes, D = gradient w.r.t. X.
#include "loss_common.h"
#include "ssim_common.h"

#define SSIM_MAX_LEVELS 5
struct SsimLayout {
  int levels, H[SSIM_MAX_LEVELS], Ho[SSIM_MAX_LEVELS], tiles[SSIM_MAX_LEVELS], pad[SSIM_MAX_LEVELS];
  long long planes, X[SSIM_MAX_LEVELS], Y[SSIM_MAX_LEVELS], D[SSIM_MAX_LEVELS], part[SSIM_MAX_LEVELS], coef, val, mm, stat, total;
  // stat: [views][8] = pred lo, hi, target lo, hi, tie-term A, tie-term B, (int) count lo, (int) count hi
};
static SsimLayout ssim_layout(long long B2, int C, int S, int p, int levels) {
  SsimLayout L;
  L.levels = levels; L.planes = B2 * C;
  long long off = 0;
  auto take = [&](long long n) { long long o = off; off += (n + 3) & ~3ll; return o; };
  int h = S;
  for (int l = 0; l < SSIM_MAX_LEVELS; ++l) {
    L.H[l] = h; L.Ho[l] = h - SSIM_R; L.pad[l] = h & 1;
    const int t = cdiv(h - SSIM_R > 0 ? h - SSIM_R : 1, SSIM_TILE);
    L.tiles[l] = t * t;
    if (l < levels) {
      L.X[l] = take(L.planes * h * h); L.Y[l] = take(L.planes * h * h); L.D[l] = take(L.planes * h * h);
      L.part[l] = take(L.planes * L.tiles[l] * 2);
    } else L.X[l] = L.Y[l] = L.D[l] = L.part[l] = 0;
    h = (h + 2 * (h & 1) - 2) / 2 + 1;  // avg_pool2d(kernel 2, stride 2, padding = h % 2)
  }
  L.coef = take(L.planes * SSIM_MAX_LEVELS * 2);
  L.val = take(L.planes);
  const long long patches = B2 * (long long)(S / p) * (S / p);
  L.mm = take(patches * 2);
  L.stat = take(2 * 8);
  L.total = off;
  return L;
}

// per-patch min / max of the prediction rows (cls row excluded, pad columns excluded)
__global__ __launch_bounds__(256) void pred_minmax_kernel(PatchGeom g, long long patches, const float* __restrict__ pred, long long ldp, float* __restrict__ mm) {
  const PatchWave w = patch_wave(g, patches);
  if (!w.live) return;
  const float* pr = pred_row(g, pred, ldp, w);
  float lo = INFINITY, hi = -INFINITY;
  for (int e = w.lane; e < g.P; e += 64) { float v = pr[e]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
  lo = -wave_max(-lo); hi = wave_max(hi);
  if (w.lane == 0) { mm[w.pt * 2] = lo; mm[w.pt * 2 + 1] = hi; }
}
__global__ __launch_bounds__(256) void ssim_stat_store_kernel(int views, int which, const float* __restrict__ mmout, float* __restrict__ stat) {
  if (threadIdx.x < views * 2) { int v = threadIdx.x >> 1, k = threadIdx.x & 1; stat[v * 8 + which * 2 + k] = mmout[v * 2 + k]; }
  if (which == 0 && threadIdx.x < views * 2) reinterpret_cast<int*>(stat)[(threadIdx.x >> 1) * 8 + 6 + (threadIdx.x & 1)] = 0;
}
// level-0 planes: X = mask * scale_01(pred), Y = mask * scale_01(target); counts the elements that attain the prediction's min / max
// (the backward of x.min() / x.max() spreads its gradient evenly over ties)
__global__ __launch_bounds__(256) void ssim_prepare_kernel(PatchGeom g, int norm_pix, long long patches, const float* __restrict__ img0,
                                                           const float* __restrict__ img1, const float* __restrict__ pred, long long ldp,
                                                           const float* __restrict__ mask, float* __restrict__ stat, float* __restrict__ X,
                                                           float* __restrict__ Y, int raw) {
  const PatchWave w = patch_wave(g, patches);
  if (!w.live) return;
  const int v = w.view;
  const float* img = patch_img(g, img0, img1, w.n2);
  float mu = 0.f, rs = 1.f;
  if (norm_pix) patch_stats(g, img, w.l, w.lane, mu, rs);
  // raw: the operands are compared as they are (util/metrics.py: images already in [0, 1]); otherwise scale_01 of each (loss family)
  const float plo = raw ? 0.f : stat[v * 8], phi = stat[v * 8 + 1], tlo = raw ? 0.f : stat[v * 8 + 2], thi = stat[v * 8 + 3];
  const float psc = raw ? 1.f : 1.f / (phi - plo + 1.0e-6f), tsc = raw ? 1.f : 1.f / (thi - tlo + 1.0e-6f);
  const float m = mask ? mask[w.pt] : 1.f;
  const float* pr = pred_row(g, pred, ldp, w);
  const int gh = w.l / g.G, gw = w.l - gh * g.G, pp = g.p * g.p;
  int nlo = 0, nhi = 0;
  for (int c = 0; c < g.C; ++c)            // channel-major walk: a wave's stores are whole p-pixel row segments of ONE plane (the element
    for (int r = w.lane; r < pp; r += 64) {  // order of a patch row interleaves the channels; its 12-byte-strided reads hit the cache)
      const int ph = r / g.p, pw = r - ph * g.p, e = r * g.C + c;
      const long long o = ((w.n2 * g.C + c) * g.S + gh * g.p + ph) * g.S + gw * g.p + pw;   // (patch_plane_offset, written out here and below: through the
      const float pv = pr[e];                                                               //  helper this loop's unrolling takes 256 VGPRs or spills SGPRs)
      nlo += pv == plo; nhi += pv == phi;
      X[o] = (pv - plo) * psc * m;
      Y[o] = ((img[((long long)c * g.S + gh * g.p + ph) * g.S + gw * g.p + pw] - mu) * rs - tlo) * tsc * m;
    }
  if (nlo) atomicAdd(reinterpret_cast<int*>(stat) + v * 8 + 6, nlo);
  if (nhi) atomicAdd(reinterpret_cast<int*>(stat) + v * 8 + 7, nhi);
}
// 2x2 average pooling with `pad` rows / columns of zeros in front (count_include_pad): both operands of one level
__global__ __launch_bounds__(256) void ssim_pool_kernel(long long planes, int H, int pad, int Hn, const float* __restrict__ X, const float* __restrict__ Y,
                                                        float* __restrict__ Xn, float* __restrict__ Yn) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= planes * Hn * Hn) return;
  const long long pl = i / ((long long)Hn * Hn); const int r = (int)(i - pl * Hn * Hn), y = r / Hn, x = r - y * Hn;
  const float* px = X + pl * H * H; const float* py = Y + pl * H * H;
  float sx = 0.f, sy = 0.f;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int yy = 2 * y - pad + dy, xx = 2 * x - pad + dx;
      if (yy >= 0 && yy < H && xx >= 0 && xx < H) { sx += px[yy * H + xx]; sy += py[yy * H + xx]; }
    }
  Xn[i] = 0.25f * sx; Yn[i] = 0.25f * sy;
}

// One 32x32 tile of the SSIM / contrast-structure maps of one plane -> part[plane][tile] = (sum ssim_map, sum cs_map)
__global__ __launch_bounds__(256) void ssim_level_fwd_kernel(SsimWin win, int H, int Ho, int tiles_x, const float* __restrict__ X, const float* __restrict__ Y,
                                                             float* __restrict__ part) {
  constexpr int T = SSIM_TILE, E = T + SSIM_R, ES = 44;  // 42 staged rows / columns, row stride 44 floats
  __shared__ __attribute__((aligned(16))) float sx[E * ES], sy[E * ES], V[5 * T * ES];
  __shared__ float red[32];
  const long long pl = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, y0 = ty * T, x0 = tx * T;
  ssim_stage<E, E / 2, ES>(X + pl * H * H, Y + pl * H * H, H, y0, x0, sx, sy);
  __syncthreads();
  ssim_pass_h<T / 4, E / 2, ES, ES, T>(win, sx, sy, V);
  __syncthreads();
  float ss = 0.f, sc = 0.f;
  if (threadIdx.x < (T / 2) * (T / 4)) {  // 16 row pairs x 8 column groups
    const int rp = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * 4;
    f2_t f[5][4];
    ssim_pass_w<5, ES, T>(win, V, rp, c0, f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f2_t mu1 = f[0][j], mu2 = f[1][j], m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
      const f2_t s1 = f[2][j] - m11, s2 = f[3][j] - m22, s12 = f[4][j] - m12;
      const f2_t cs = (s12 * 2.f + SSIM_C2) * rcp2(s1 + s2 + SSIM_C2);
      const f2_t sm = (m12 * 2.f + SSIM_C1) * rcp2(m11 + m22 + SSIM_C1) * cs;
      if (x0 + c0 + j < Ho) {
        if (y0 + 2 * rp < Ho) { ss += sm[0]; sc += cs[0]; }
        if (y0 + 2 * rp + 1 < Ho) { ss += sm[1]; sc += cs[1]; }
      }
    }
  }
  ss = block_sum(ss, red); sc = block_sum(sc, red);
  if (threadIdx.x == 0) { part[(pl * gridDim.x + blockIdx.x) * 2] = ss; part[(pl * gridDim.x + blockIdx.x) * 2 + 1] = sc; }
}
// Per-plane means -> per-plane score -> per-view loss term, and the coefficients the backward needs:
//   d(term_v) / d(mean ssim_map of level l, plane) = coef[plane][l][0],  d / d(mean cs_map) = coef[plane][l][1]   (already / Ho^2)
// ssim: relu(mean) per plane (nonnegative_ssim), averaged.  ms_ssim: prod_l relu(.)^w_l with cs for l < 4 and ssim for l = 4; a
// clamped factor zeroes the product and (threshold backward selects 0) every gradient of that plane.
struct SsimStatArgs { int levels, tiles[SSIM_MAX_LEVELS], Ho[SSIM_MAX_LEVELS]; const float* part[SSIM_MAX_LEVELS]; };
__global__ __launch_bounds__(256) void ssim_stats_kernel(SsimStatArgs a, long long planes, int views, float* __restrict__ coef, float* __restrict__ val,
                                                         int signed_ssim) {
  const float wts[5] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};
  const long long per_view = planes / views;
  // one wave per plane: the tile partials of a level are summed across the lanes (fixed order: deterministic)
  const long long pl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pl >= planes) return;
  float ms[SSIM_MAX_LEVELS], mc[SSIM_MAX_LEVELS];
#pragma unroll
  for (int l = 0; l < SSIM_MAX_LEVELS; ++l) {
    ms[l] = mc[l] = 0.f;
    if (l < a.levels) {
      float s = 0.f, c = 0.f;
      for (int t = lane; t < a.tiles[l]; t += 64) { s += a.part[l][(pl * a.tiles[l] + t) * 2]; c += a.part[l][(pl * a.tiles[l] + t) * 2 + 1]; }
      const float inv = 1.f / ((float)a.Ho[l] * a.Ho[l]);
      ms[l] = wave_sum(s) * inv; mc[l] = wave_sum(c) * inv;
    }
  }
  if (lane != 0) return;
  float cf[SSIM_MAX_LEVELS * 2];
#pragma unroll
  for (int l = 0; l < SSIM_MAX_LEVELS * 2; ++l) cf[l] = 0.f;
  const float base = -1.f / (float)per_view;
  float v;
  if (a.levels == 1) {
    v = signed_ssim ? ms[0] : fmaxf(ms[0], 0.f);   // nonnegative_ssim=True in the loss (MAE_ViT_Shared.py:204-206), False in util/metrics.py
    cf[0] = (signed_ssim || ms[0] > 0.f) ? base / ((float)a.Ho[0] * a.Ho[0]) : 0.f;
  } else {
    float t[SSIM_MAX_LEVELS]; bool pos = true;
    v = 1.f;
#pragma unroll
    for (int l = 0; l < SSIM_MAX_LEVELS; ++l) { t[l] = fmaxf(l == SSIM_MAX_LEVELS - 1 ? ms[l] : mc[l], 0.f); pos &= t[l] > 0.f; v *= powf(t[l], wts[l]); }
    if (!pos) v = 0.f;
#pragma unroll
    for (int l = 0; l < SSIM_MAX_LEVELS; ++l)
      cf[l * 2 + (l == SSIM_MAX_LEVELS - 1 ? 0 : 1)] = pos ? base * wts[l] * v / t[l] / ((float)a.Ho[l] * a.Ho[l]) : 0.f;
  }
#pragma unroll
  for (int l = 0; l < SSIM_MAX_LEVELS * 2; ++l) coef[pl * SSIM_MAX_LEVELS * 2 + l] = cf[l];
  val[pl] = v;
}
__global__ __launch_bounds__(1024) void ssim_terms_kernel(long long per_view, int views, const float* __restrict__ val, float* __restrict__ terms) {
  __shared__ float red[32];
  for (int vw = 0; vw < views; ++vw) {
    float s = 0.f;
    for (long long i = threadIdx.x; i < per_view; i += blockDim.x) s += val[vw * per_view + i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) terms[vw] = 1.f - s / (float)per_view;
  }
}
// Gradient of one level w.r.t. its X plane, for one 32x32 tile of pixels:
//   dX(p) = sum_q w(p - q) [G0(q) + 2 X(p) G1(q) + Y(p) G2(q)]  (+ 1/4 of the next level's gradient at the pooled position)
// with, at every window position q (F = cs * (a * lum + b) is what the plane's score depends on):
//   c = a lum + b,  G1 = dF/dE[xx] = -c cs / B2,  G2 = dF/dE[xy] = 2 c / B2,  G0 = dF/dmu1 = a cs (2 mu2 - 2 lum mu1) / B1 - 2 mu1 G1 - mu2 G2
__global__ __launch_bounds__(256) void ssim_level_bwd_kernel(SsimWin win, int H, int Ho, int tiles_x, int lvl, const float* __restrict__ X,
                                                             const float* __restrict__ Y, const float* __restrict__ coef,
                                                             const float* __restrict__ Dn, int Hn, int pad, float* __restrict__ D) {
  // window positions q of this tile: 42 x 42 (q = p - 10 .. p), padded to 44 so that every pass works on groups of four
  constexpr int T = SSIM_TILE, E1P = 44, E2 = E1P + SSIM_R, S2 = 56, S1 = 44;
  __shared__ __attribute__((aligned(16))) float sxy[2 * E2 * S2];  // X | Y over the 54 x 54 halo region, later G[3][44][44]
  __shared__ __attribute__((aligned(16))) float V[5 * E1P * S2];   // H-filtered quantities [5][44][56], later Tt[3][32][44]
  static_assert(3 * E1P * S1 <= 2 * E2 * S2 && 3 * T * S1 <= 5 * E1P * S2, "aliases fit");
  float* sx = sxy; float* sy = sxy + E2 * S2;
  const long long pl = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, y0 = ty * T, x0 = tx * T;
  const float* px = X + pl * H * H; const float* py = Y + pl * H * H;
  const float ca = coef[pl * SSIM_MAX_LEVELS * 2 + lvl * 2], cb = coef[pl * SSIM_MAX_LEVELS * 2 + lvl * 2 + 1];
  ssim_stage<E2, E2 / 2, S2>(px, py, H, y0 - SSIM_R, x0 - SSIM_R, sx, sy);
  __syncthreads();
  ssim_pass_h<E1P / 4, E2 / 2, S2, S2, E1P>(win, sx, sy, V);   // window rows q = y0 - 10 + r
  __syncthreads();
  float* G = sxy;
  if (threadIdx.x < (E1P / 2) * (E1P / 4)) {  // 22 row pairs x 11 column groups: along W, then the three coefficient maps
    const int rp = threadIdx.x / (E1P / 4), c0 = (threadIdx.x - rp * (E1P / 4)) * 4, qy = y0 - SSIM_R + 2 * rp;
    f2_t f[5][4];
    ssim_pass_w<5, S2, E1P>(win, V, rp, c0, f);
    const bool oky0 = qy >= 0 && qy < Ho, oky1 = qy + 1 >= 0 && qy + 1 < Ho;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int qx = x0 - SSIM_R + c0 + j;
      const f2_t mu1 = f[0][j], mu2 = f[1][j], m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
      const f2_t s1 = f[2][j] - m11, s2 = f[3][j] - m22, s12 = f[4][j] - m12;
      const f2_t rB1 = rcp2(m11 + m22 + SSIM_C1), rB2 = rcp2(s1 + s2 + SSIM_C2);
      const f2_t lum = (m12 * 2.f + SSIM_C1) * rB1, cs = (s12 * 2.f + SSIM_C2) * rB2;
      const f2_t cc = lum * ca + cb;
      f2_t g1 = -cc * cs * rB2;
      f2_t g2 = cc * rB2 * 2.f;
      f2_t g0 = cs * (mu2 - lum * mu1) * rB1 * (2.f * ca) - mu1 * g1 * 2.f - mu2 * g2;
      const bool okx = qx >= 0 && qx < Ho;
      if (!(okx && oky0)) { g0[0] = 0.f; g1[0] = 0.f; g2[0] = 0.f; }
      if (!(okx && oky1)) { g0[1] = 0.f; g1[1] = 0.f; g2[1] = 0.f; }
      float* g = G + (2 * rp) * S1 + c0 + j;
      g[0] = g0[0]; g[S1] = g0[1];
      g[E1P * S1] = g1[0]; g[E1P * S1 + S1] = g1[1];
      g[2 * E1P * S1] = g2[0]; g[2 * E1P * S1 + S1] = g2[1];
    }
  }
  __syncthreads();
  float* Tt = V;
  for (int i = threadIdx.x; i < 3 * (T / 4) * (E1P / 2); i += 256) {  // transposed filter along H: pixel rows p = y0 + r take windows q = p - k
    const int m = i / ((T / 4) * (E1P / 2)), j = i - m * (T / 4) * (E1P / 2), rg = j / (E1P / 2), cp = j - rg * (E1P / 2);
    f2_t in[4 + SSIM_R], o[4];
#pragma unroll
    for (int k = 0; k < 4 + SSIM_R; ++k) in[k] = *reinterpret_cast<const f2_t*>(G + (m * E1P + rg * 4 + k) * S1 + 2 * cp);   // (symmetric window: G rows r .. r + 10 of pixel row r)
    fir4(win, in, o);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) *reinterpret_cast<f2_t*>(Tt + (m * T + rg * 4 + jj) * S1 + 2 * cp) = o[jj];
  }
  __syncthreads();
  if (threadIdx.x < (T / 2) * (T / 4)) {
    float* pd = D + pl * H * H;
    const float* pn = Dn ? Dn + pl * Hn * Hn : nullptr;
    const int rp = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * 4;
    f2_t o[3][4];
    ssim_pass_w<3, S1, T>(win, Tt, rp, c0, o);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int gy = y0 + 2 * rp + h;
      if (gy >= H) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int gx = x0 + c0 + j;
        if (gx >= H) continue;
        float d = o[0][j][h] + 2.f * px[(long long)gy * H + gx] * o[1][j][h] + py[(long long)gy * H + gx] * o[2][j][h];
        if (pn) { const int yy = (gy + pad) >> 1, xx = (gx + pad) >> 1; if (yy < Hn && xx < Hn) d += 0.25f * pn[yy * Hn + xx]; }
        pd[(long long)gy * H + gx] = d;
      }
    }
  }
}
// extra[pt][e] = gout * scale * dX0 * mask / range  (d loss / d pred through the scaled value), per-patch partial sums of the two
// terms that flow into the tensor's min and max:  A = sum dxs (xs - 1) / range,  B = -sum dxs xs / range
__global__ __launch_bounds__(256) void ssim_pred_bwd_kernel(PatchGeom g, long long patches, const float* __restrict__ pred, long long ldp,
                                                            const float* __restrict__ mask, const float* __restrict__ stat, const float* __restrict__ D0,
                                                            const float* __restrict__ gout, float scale, float* __restrict__ extra, float* __restrict__ ab) {
  const PatchWave w = patch_wave(g, patches);
  if (!w.live) return;
  const int lane = w.lane, v = w.view;
  const float m = mask ? mask[w.pt] : 1.f;
  float* ex = extra + w.pt * g.P;
  float A = 0.f, B = 0.f;
  if (m == 0.f) { for (int e = lane; e < g.P; e += 64) ex[e] = 0.f; }
  else {
    const float plo = stat[v * 8], psc = 1.f / (stat[v * 8 + 1] - plo + 1.0e-6f), gs = gout[0] * scale * m;
    const float* pr = pred_row(g, pred, ldp, w);
    for (int e = lane; e < g.P; e += 64) {
      const float dxs = D0[patch_elem_offset(g, w.n2, w.l, e)] * gs;
      const float xs = (pr[e] - plo) * psc;
      ex[e] = dxs * psc;
      A += dxs * (xs - 1.f) * psc; B -= dxs * xs * psc;
    }
  }
  A = wave_sum(A); B = wave_sum(B);
  if (lane == 0) { ab[w.pt * 2] = A; ab[w.pt * 2 + 1] = B; }
}
__global__ __launch_bounds__(1024) void ssim_tie_reduce_kernel(long long per_view, int views, const float* __restrict__ ab, float* __restrict__ stat) {
  __shared__ float red[32];
  for (int v = 0; v < views; ++v) {
    float A = 0.f, B = 0.f;
    for (long long i = threadIdx.x; i < per_view; i += blockDim.x) { A += ab[(v * per_view + i) * 2]; B += ab[(v * per_view + i) * 2 + 1]; }
    A = block_sum(A, red); B = block_sum(B, red);
    if (threadIdx.x == 0) {
      const int* cnt = reinterpret_cast<const int*>(stat) + v * 8 + 6;
      stat[v * 8 + 4] = A / (float)max(cnt[0], 1); stat[v * 8 + 5] = B / (float)max(cnt[1], 1);
    }
  }
}
__global__ __launch_bounds__(256) void ssim_tie_apply_kernel(PatchGeom g, long long patches, const float* __restrict__ pred, long long ldp,
                                                             const float* __restrict__ stat, float* __restrict__ extra) {
  const PatchWave w = patch_wave(g, patches);
  if (!w.live) return;
  const int v = w.view;
  const float plo = stat[v * 8], phi = stat[v * 8 + 1], A = stat[v * 8 + 4], B = stat[v * 8 + 5];
  const float* pr = pred_row(g, pred, ldp, w);
  for (int e = w.lane; e < g.P; e += 64) {
    const float pv = pr[e];
    if (pv == plo || pv == phi) extra[w.pt * g.P + e] += (pv == plo ? A : 0.f) + (pv == phi ? B : 0.f);
  }
}
// losses[] patch-up after csmae_loss_finalize: the ssim term of each view joins (weight 0.1, the mse_* kinds) or replaces the
// masked per-patch term
__global__ void ssim_apply_kernel(int pure, int views, float weight, float recon_scale, const float* __restrict__ terms, float* __restrict__ losses) {
  if (threadIdx.x != 0) return;
  float add = 0.f;
  for (int v = 0; v < views; ++v) {
    const float t = weight * terms[v];
    if (pure) losses[1 + v] = t; else losses[1 + v] += t;
    add += t;
  }
  losses[0] = (pure ? losses[3] + losses[4] + losses[5] : losses[0]) + recon_scale * add;
}

extern "C" int csmae_ssim_workspace_floats(long long B2, int C, int S, int p, int levels, long long* floats) {
  CSMAE_REQUIRE(B2 > 0 && C > 0 && S > 0 && p > 0 && S % p == 0 && (levels == 1 || levels == SSIM_MAX_LEVELS) && floats, "csmae_ssim_workspace_floats: bad args");
  *floats = ssim_layout(B2, C, S, p, levels).total;
  return CSMAE_OK;
}
extern "C" int csmae_ssim_fwd(int levels, int flags, int norm_pix, long long B2, int N, int C, int S, int p, const float* img0, const float* img1,
                              const float* pred, long long ldp, const float* mask, float* ws, float* terms, void* stream) {
  CSMAE_REQUIRE(flags >= 0 && flags <= 3, "csmae_ssim_fwd: bad flags %d", flags);
  CSMAE_REQUIRE(levels == 1 || levels == SSIM_MAX_LEVELS, "csmae_ssim_fwd: levels must be 1 (ssim) or 5 (ms_ssim)");
  CSMAE_REQUIRE(B2 > 0 && N > 0 && B2 % N == 0 && B2 / N <= 2 && S % p == 0 && ws && terms && pred && img0, "csmae_ssim_fwd: bad args");
  CSMAE_REQUIRE(S >= SSIM_WIN, "csmae_ssim_fwd: images smaller than the 11-tap window are not supported (S = %d)", S);
  CSMAE_REQUIRE(levels == 1 || S > SSIM_R * 16, "csmae_ssim_fwd: Image size should be larger than 160 due to the 4 downsamplings in ms-ssim (S = %d)", S);
  hipStream_t st = (hipStream_t)stream;
  const PatchGeom g = make_geom(N, C, S, p);
  const SsimLayout L = ssim_layout(B2, C, S, p, levels);
  const SsimWin win = ssim_window();
  const long long patches = B2 * g.L;
  const int views = (int)(B2 / N);
  float* stat = ws + L.stat; float* mm = ws + L.mm; float* mmout = ws + L.val;  // (val is free until the stats kernel)
  hipLaunchKernelGGL(pred_minmax_kernel, dim3(cdiv(patches, 4)), dim3(256), 0, st, g, patches, pred, ldp, mm);
  loss_launch_minmax_reduce((long long)N * g.L, views, mm, mmout, st);
  hipLaunchKernelGGL(ssim_stat_store_kernel, dim3(1), dim3(64), 0, st, views, 0, mmout, stat);
  loss_launch_target_minmax(g, norm_pix, patches, img0, img1, mm, st);
  loss_launch_minmax_reduce((long long)N * g.L, views, mm, mmout, st);
  hipLaunchKernelGGL(ssim_stat_store_kernel, dim3(1), dim3(64), 0, st, views, 1, mmout, stat);
  hipLaunchKernelGGL(ssim_prepare_kernel, dim3(cdiv(patches, 4)), dim3(256), 0, st, g, norm_pix, patches, img0, img1, pred, ldp, mask, stat, ws + L.X[0], ws + L.Y[0], flags & 1);
  SsimStatArgs sa; sa.levels = levels;
  for (int l = 0; l < SSIM_MAX_LEVELS; ++l) { sa.tiles[l] = L.tiles[l]; sa.Ho[l] = L.Ho[l]; sa.part[l] = ws + L.part[l]; }
  for (int l = 0; l < levels; ++l) {
    const int tx = cdiv(L.Ho[l], SSIM_TILE);
    hipLaunchKernelGGL(ssim_level_fwd_kernel, dim3(tx * tx, (unsigned)L.planes), dim3(256), 0, st, win, L.H[l], L.Ho[l], tx, ws + L.X[l], ws + L.Y[l], ws + L.part[l]);
    if (l + 1 < levels)
      hipLaunchKernelGGL(ssim_pool_kernel, dim3(cdiv(L.planes * L.H[l + 1] * L.H[l + 1], 256)), dim3(256), 0, st, L.planes, L.H[l], L.pad[l], L.H[l + 1],
                         ws + L.X[l], ws + L.Y[l], ws + L.X[l + 1], ws + L.Y[l + 1]);
  }
  hipLaunchKernelGGL(ssim_stats_kernel, dim3(cdiv(L.planes, 4)), dim3(256), 0, st, sa, L.planes, views, ws + L.coef, ws + L.val, (flags >> 1) & 1);
  hipLaunchKernelGGL(ssim_terms_kernel, dim3(1), dim3(1024), 0, st, L.planes / views, views, ws + L.val, terms);
  return csmae_check_launch("csmae_ssim_fwd");
}
extern "C" int csmae_ssim_apply(int pure, int views, float weight, float recon_scale, const float* terms, float* losses, void* stream) {
  CSMAE_REQUIRE((views == 1 || views == 2) && terms && losses, "csmae_ssim_apply: bad args");
  hipLaunchKernelGGL(ssim_apply_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, pure, views, weight, recon_scale, terms, losses);
  return csmae_check_launch("csmae_ssim_apply");
}
extern "C" int csmae_ssim_bwd(int levels, long long B2, int N, int C, int S, int p, const float* pred, long long ldp, const float* mask,
                              const float* gout, float scale, float* ws, float* extra, void* stream) {
  CSMAE_REQUIRE(levels == 1 || levels == SSIM_MAX_LEVELS, "csmae_ssim_bwd: levels must be 1 (ssim) or 5 (ms_ssim)");
  CSMAE_REQUIRE(B2 > 0 && N > 0 && B2 % N == 0 && B2 / N <= 2 && S % p == 0 && ws && extra && pred && gout, "csmae_ssim_bwd: bad args");
  hipStream_t st = (hipStream_t)stream;
  const PatchGeom g = make_geom(N, C, S, p);
  const SsimLayout L = ssim_layout(B2, C, S, p, levels);
  const SsimWin win = ssim_window();
  const long long patches = B2 * g.L;
  const int views = (int)(B2 / N);
  for (int l = levels - 1; l >= 0; --l) {
    const int tx = cdiv(L.H[l], SSIM_TILE);
    const bool nxt = l + 1 < levels;
    hipLaunchKernelGGL(ssim_level_bwd_kernel, dim3(tx * tx, (unsigned)L.planes), dim3(256), 0, st, win, L.H[l], L.Ho[l], tx, l, ws + L.X[l], ws + L.Y[l],
                       ws + L.coef, nxt ? ws + L.D[l + 1] : nullptr, nxt ? L.H[l + 1] : 0, L.pad[l], ws + L.D[l]);
  }
  hipLaunchKernelGGL(ssim_pred_bwd_kernel, dim3(cdiv(patches, 4)), dim3(256), 0, st, g, patches, pred, ldp, mask, ws + L.stat, ws + L.D[0], gout, scale, extra, ws + L.mm);
  hipLaunchKernelGGL(ssim_tie_reduce_kernel, dim3(1), dim3(1024), 0, st, (long long)N * g.L, views, ws + L.mm, ws + L.stat);
  hipLaunchKernelGGL(ssim_tie_apply_kernel, dim3(cdiv(patches, 4)), dim3(256), 0, st, g, patches, pred, ldp, ws + L.stat, extra);
  return csmae_check_launch("csmae_ssim_bwd");
}
