// Per-image reconstruction scores of a whole batch (util/metrics.py batch_metrics, util/viz.py run_eval): with X = img * std + mean and
// Y = the un-patchified prediction * std + mean,  out[n] = { sum (X - Y)^2, sum |X - Y|, ssim(X, Y), 0 }.  ssim is pytorch-msssim 0.2.1's
// (11-tap gaussian, sigma 1.5, "valid" windows, data_range 1, signed), the mean over the image's C planes — what util.metrics.calc_ssim gives
// for that one image.  Nothing needs a backward, so no plane is written to HBM: a workgroup fills its 42 x 42 window of both operands straight
// from the image and from the patch rows, un-normalising on the way into LDS, and runs the FIR passes of ssim_common.h on it.
//   recon_eval_tile_kernel   one workgroup per (32 x 32 tile of the Ho x Ho ssim map, plane): part[plane][tile] = (sum ssim_map, sse, sae)
//   recon_eval_fold_kernel   one wave per image: its C * tiles partials in a fixed order -> out[n]
// No atomics, fixed orders: an image's four floats depend on that image alone, not on N or on its place in the batch.
#include "ssim_common.h"

#define RE_WAVES 4   // images per workgroup of the fold

// n / p and n % p for 0 <= n < S: multiply-shift when S * p < 2^24 (mp = ceil(2^24 / p), exact there), a division otherwise (mp = 0)
struct ReGeom { int C, S, p, G, Ho, tiles_x, tiles; unsigned mp; };
__device__ __forceinline__ int re_div_p(const ReGeom& g, int n) { return g.mp ? (int)(((unsigned long long)(unsigned)n * g.mp) >> 24) : n / g.p; }

// Pixel ownership of the element sums.  The windows of neighbouring tiles overlap by 10 rows / columns, and the ssim map (Ho = S - 10) has fewer
// rows than the image, so the sums cannot simply follow the staged window: a tile owns the 32 rows [y0, y0 + 32) it owns of the map, and the LAST
// tile of an axis also owns the rows behind them, through S - 1 (y0 + 32 >= Ho there, so y0 + 42 >= S: its halo covers them).  Columns alike.
// Every pixel is then counted exactly once.
template <typename TP>
__global__ __launch_bounds__(256) void recon_eval_tile_kernel(SsimWin win, ReGeom g, const float* __restrict__ img, const TP* __restrict__ pred, long long ldp,
                                                              long long img_stride, const float* __restrict__ mean, const float* __restrict__ std,
                                                              float* __restrict__ part) {
  constexpr int T = SSIM_TILE, E = T + SSIM_R, ES = 44;  // 42 staged rows / columns, row stride 44 floats
  __shared__ __attribute__((aligned(16))) float sx[E * ES], sy[E * ES], V[5 * T * ES];
  __shared__ float red[32];
  const long long pl = blockIdx.x / g.tiles;             // plane = n * C + c
  const int tile = (int)(blockIdx.x - pl * g.tiles);
  const long long n = pl / g.C;
  const int c = (int)(pl - n * g.C);
  const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x, y0 = ty * T, x0 = tx * T;
  const bool last_y = ty == g.tiles_x - 1, last_x = tx == g.tiles_x - 1;
  const float sd = std[c], mn = mean[c];
  const float* pi = img + pl * g.S * g.S;
  const TP* pp = pred + n * img_stride;
  float sse = 0.f, sae = 0.f;
  for (int i = threadIdx.x; i < E * E; i += 256) {
    const int r = i / E, cx = i - r * E, gy = y0 + r, gx = x0 + cx;
    float x = 0.f, y = 0.f;   // (zero outside the image: such a value only reaches windows outside the Ho x Ho map)
    if (gy < g.S && gx < g.S) {
      const int gh = re_div_p(g, gy), ph = gy - gh * g.p, gw = re_div_p(g, gx), pw = gx - gw * g.p;
      x = pi[(long long)gy * g.S + gx] * sd + mn;
      y = ld_as_f32<TP>(pp + ((long long)gh * g.G + gw) * ldp + (ph * g.p + pw) * g.C + c) * sd + mn;
      if ((r < T || last_y) && (cx < T || last_x)) { const float d = x - y; sse += d * d; sae += fabsf(d); }
    }
    sx[r * ES + cx] = x; sy[r * ES + cx] = y;
  }
  __syncthreads();
  ssim_pass_h<T / 4, E / 2, ES, ES, T>(win, sx, sy, V);
  __syncthreads();
  float ss = 0.f;
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
      if (x0 + c0 + j < g.Ho) {
        if (y0 + 2 * rp < g.Ho) ss += sm[0];
        if (y0 + 2 * rp + 1 < g.Ho) ss += sm[1];
      }
    }
  }
  ss = block_sum(ss, red); sse = block_sum(sse, red); sae = block_sum(sae, red);
  if (threadIdx.x == 0) { float* o = part + (long long)blockIdx.x * 3; o[0] = ss; o[1] = sse; o[2] = sae; }
}

// part is [N][C * tiles][3]: lane j adds partials j, j + 64, ... in that order, then the wave tree
__global__ __launch_bounds__(64 * RE_WAVES) void recon_eval_fold_kernel(long long N, int per_image, float inv_count, const float* __restrict__ part, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long n = (long long)blockIdx.x * RE_WAVES + (threadIdx.x >> 6);
  if (n >= N) return;   // (whole waves leave: no barrier follows)
  const float* q = part + n * per_image * 3;
  float ss = 0.f, sse = 0.f, sae = 0.f;
  for (int t = lane; t < per_image; t += 64) { ss += q[t * 3]; sse += q[t * 3 + 1]; sae += q[t * 3 + 2]; }
  ss = wave_sum(ss); sse = wave_sum(sse); sae = wave_sum(sae);
  if (lane < 4) out[n * 4 + lane] = lane == 0 ? sse : lane == 1 ? sae : lane == 2 ? ss * inv_count : 0.f;
}

static int re_tiles_x(int S) { return cdiv(S - SSIM_R, SSIM_TILE); }

extern "C" int csmae_recon_eval_workspace_floats(long long N, int C, int S, long long* floats) {
  CSMAE_REQUIRE(N > 0 && C >= 1 && floats, "csmae_recon_eval_workspace_floats: null or empty argument");
  CSMAE_REQUIRE(S >= SSIM_WIN, "csmae_recon_eval_workspace_floats: images smaller than the 11-tap window are not supported (S = %d)", S);
  const long long t = re_tiles_x(S);
  *floats = N * C * t * t * 3;
  return CSMAE_OK;
}
extern "C" int csmae_recon_eval(int pred_dtype, long long N, int C, int S, int p, const float* img, const void* pred, long long ldp, long long img_stride,
                                const float* mean, const float* std, float* part, float* out, void* stream) {
  CSMAE_REQUIRE(pred_dtype == CSMAE_F32 || pred_dtype == CSMAE_BF16, "csmae_recon_eval: the prediction is fp32 or bf16 (pred_dtype %d)", pred_dtype);
  CSMAE_REQUIRE(img && pred && mean && std && part && out, "csmae_recon_eval: null argument");
  CSMAE_REQUIRE(N > 0 && C >= 1 && p >= 1, "csmae_recon_eval: N = %lld, C = %d, p = %d must be positive", N, C, p);
  CSMAE_REQUIRE(S >= SSIM_WIN, "csmae_recon_eval: images smaller than the 11-tap window are not supported (S = %d)", S);
  CSMAE_REQUIRE(S % p == 0, "csmae_recon_eval: the patch size %d does not tile the image (S = %d)", p, S);
  const long long G = S / p, P = (long long)p * p * C;
  CSMAE_REQUIRE(P <= 0x7fffffffLL && ldp >= P, "csmae_recon_eval: ldp = %lld must cover the %lld elements of a patch row", ldp, P);
  CSMAE_REQUIRE(N == 1 || img_stride >= (G * G - 1) * ldp + P, "csmae_recon_eval: img_stride = %lld is less than one image's patch rows", img_stride);
  ReGeom g;
  g.C = C; g.S = S; g.p = p; g.G = (int)G; g.Ho = S - SSIM_R; g.tiles_x = re_tiles_x(S); g.tiles = g.tiles_x * g.tiles_x;
  g.mp = (long long)S * p < (1ll << 24) ? (unsigned)(((1ull << 24) + p - 1) / p) : 0u;
  const long long blocks = N * C * g.tiles, per_image = (long long)C * g.tiles;
  CSMAE_REQUIRE(blocks <= 0x7fffffffLL && per_image * 3 <= 0x7fffffffLL, "csmae_recon_eval: %lld tiles are beyond the grid", blocks);
  hipStream_t st = (hipStream_t)stream;
  const SsimWin win = ssim_window();
  if (pred_dtype == CSMAE_F32)
    hipLaunchKernelGGL(recon_eval_tile_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, win, g, img, (const float*)pred, ldp, img_stride, mean, std, part);
  else
    hipLaunchKernelGGL(recon_eval_tile_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, win, g, img, (const bf16_t*)pred, ldp, img_stride, mean, std, part);
  const float inv_count = 1.f / ((float)C * (float)g.Ho * (float)g.Ho);
  hipLaunchKernelGGL(recon_eval_fold_kernel, dim3(cdiv(N, RE_WAVES)), dim3(64 * RE_WAVES), 0, st, N, (int)per_image, inv_count, part, out);
  return csmae_check_launch("csmae_recon_eval");
}
