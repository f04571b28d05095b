// Reconstruction contact sheets of a whole batch (util/viz.py reconstruction_panels, plot_reconstruction, run_eval): for every image one RGB row
// of K panels, side by side with `gap` white pixels between them, as bytes ready to be saved: out [N][S][W][3], W = K S + (K - 1) gap.  With
// X = img * std + mean, Y = the un-patchified prediction * std + mean and m = the mask value of the pixel's patch (1 = removed), a panel shows
//   0 x: X    1 xm: X (1 - m)    2 y: Y    3 ym: Y m    4 xm_ym: X (1 - m) + Y m      (the five arrays of util.viz.run_one_image, in its order)
// of the three channels band_r, band_g, band_b, each as byte = (int) min(max(255 v, 0), 255) (the reference's plot_image), 0 for a NaN.
// Straight from the operands csmae_recon_eval reads: no fp32 plane goes to memory.
//
// Store scheme.  The row stride 3 W is in general no multiple of 4 and an image's sheet starts wherever the one before it ends, so rows cannot be
// the unit of an aligned store.  An image's sheet is instead ONE flat range of B = 3 W S bytes: lane j of the image owns the j-th ALIGNED dword that
// touches the range, finds (row, column, channel) of the dword's first byte with two divisions, walks the other three by increments, and stores the
// dword whole.  Only the first and the last dword of an image can hang over its ends: their inside bytes leave as byte stores, so the neighbouring
// image (or the caller's memory around the buffer) is never touched and every byte is written exactly once.  A wave stores 256 contiguous bytes.
// No atomics; an image's bytes depend on that image alone.
#include "common.h"

struct RpGeom {
  int C, S, p, G, PW, W3;   // PW = S + gap: a panel and the gap behind it; W3 = 3 W: bytes of a sheet row
  unsigned B, bpi;          // bytes of one image's sheet; workgroups per image
  int br, bg, bb;           // the channels shown as red, green, blue
  unsigned codes;           // panel k's code in bits [4 k, 4 k + 4)
};

// truncating, clamped, defined for every input: a NaN fails the first comparison (0), +inf the second (255)
__device__ __forceinline__ unsigned rp_to_byte(float v) {
  const float t = v * 255.f;
  return t >= 0.f ? (t < 255.f ? (unsigned)(int)t : 255u) : 0u;
}

template <typename TP>
__device__ __forceinline__ unsigned rp_value(const RpGeom& g, const float* __restrict__ pi, const TP* __restrict__ pp, long long ldp, const float* __restrict__ pm,
                                             const float* __restrict__ mean, const float* __restrict__ std, unsigned y, unsigned col, unsigned ch) {
  const unsigned k = col / (unsigned)g.PW, x = col - k * g.PW;
  if (x >= (unsigned)g.S) return 255u;   // the gap
  const unsigned code = (g.codes >> (4 * k)) & 15u;
  const int c = ch == 0 ? g.br : ch == 1 ? g.bg : g.bb;
  const float sd = std[c], mn = mean[c];
  const unsigned gh = y / (unsigned)g.p, gw = x / (unsigned)g.p, l = gh * g.G + gw;
  float X = 0.f, Y = 0.f, m = 0.f;   // (an operand a panel does not show is not read: its NaNs cannot reach the byte)
  if (code != 2 && code != 3) X = pi[((long long)c * g.S + y) * g.S + x] * sd + mn;
  if (code >= 2) Y = ld_as_f32<TP>(pp + (long long)l * ldp + ((y - gh * g.p) * g.p + (x - gw * g.p)) * g.C + c) * sd + mn;
  if (code != 0 && code != 2) m = pm[l];
  const float v = code == 0 ? X : code == 1 ? X * (1.f - m) : code == 2 ? Y : code == 3 ? Y * m : X * (1.f - m) + Y * m;
  return rp_to_byte(v);
}

template <typename TP>
__global__ __launch_bounds__(256) void recon_panel_kernel(RpGeom g, const float* __restrict__ img, const TP* __restrict__ pred, long long ldp, long long img_stride,
                                                          const float* __restrict__ mask, const float* __restrict__ mean, const float* __restrict__ std,
                                                          unsigned char* __restrict__ out) {
  const long long n = blockIdx.x / g.bpi;
  const unsigned j = (unsigned)(blockIdx.x - n * g.bpi) * 256u + threadIdx.x;
  unsigned char* po = out + n * (long long)g.B;
  const long long o0 = 4ll * j - (long long)((uintptr_t)po & 3);   // offset in the sheet of the first byte of aligned dword j: -3 .. B + 2
  if (o0 >= (long long)g.B) return;
  const float* pi = img + n * g.C * g.S * g.S;
  const TP* pp = pred + n * img_stride;
  const float* pm = mask + n * g.G * g.G;
  const unsigned first = o0 < 0 ? 0u : (unsigned)o0;
  unsigned y = first / (unsigned)g.W3, r = first - y * g.W3, col = r / 3u, ch = r - col * 3u;
  unsigned word = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const long long o = o0 + b;
    if (o < 0 || o >= (long long)g.B) continue;
    word |= rp_value<TP>(g, pi, pp, ldp, pm, mean, std, y, col, ch) << (8 * b);
    if (++ch == 3u) { ch = 0; ++col; }
    if (++r == (unsigned)g.W3) { r = 0; col = 0; ++y; }
  }
  if (o0 >= 0 && o0 + 4 <= (long long)g.B) {
    *reinterpret_cast<unsigned*>(po + o0) = word;
  } else {
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (o0 + b >= 0 && o0 + b < (long long)g.B) po[o0 + b] = (unsigned char)(word >> (8 * b));
  }
}

extern "C" int csmae_recon_panel(int pred_dtype, long long N, int C, int S, int p, const float* img, const void* pred, long long ldp, long long img_stride,
                                 const float* mask, const float* mean, const float* std, int band_r, int band_g, int band_b, int panel0, int panel1, int panel2,
                                 int panel3, int panel4, int n_panels, int gap, unsigned char* out, void* stream) {
  CSMAE_REQUIRE(pred_dtype == CSMAE_F32 || pred_dtype == CSMAE_BF16, "csmae_recon_panel: the prediction is fp32 or bf16 (pred_dtype %d)", pred_dtype);
  CSMAE_REQUIRE(img && pred && mask && mean && std && out, "csmae_recon_panel: null argument (img, pred, mask, mean, std or out)");
  CSMAE_REQUIRE(N > 0 && C >= 1 && p >= 1 && S >= 1, "csmae_recon_panel: N = %lld, C = %d, S = %d, p = %d must be positive", N, C, S, p);
  CSMAE_REQUIRE(S % p == 0, "csmae_recon_panel: the patch size %d does not tile the image (S = %d)", p, S);
  const long long G = S / p, P = (long long)p * p * C;
  CSMAE_REQUIRE(P <= 0x7fffffffLL && ldp >= P, "csmae_recon_panel: ldp = %lld must cover the %lld elements of a patch row", ldp, P);
  CSMAE_REQUIRE(N == 1 || img_stride >= (G * G - 1) * ldp + P, "csmae_recon_panel: img_stride = %lld is less than one image's patch rows", img_stride);
  CSMAE_REQUIRE(band_r >= 0 && band_r < C && band_g >= 0 && band_g < C && band_b >= 0 && band_b < C,
                "csmae_recon_panel: band_r, band_g, band_b = %d, %d, %d must lie in [0, C = %d)", band_r, band_g, band_b, C);
  CSMAE_REQUIRE(n_panels >= 1 && n_panels <= 5, "csmae_recon_panel: n_panels = %d must lie in [1, 5]", n_panels);
  const int code[5] = {panel0, panel1, panel2, panel3, panel4};
  unsigned codes = 0;
  for (int k = 0; k < n_panels; ++k) {
    CSMAE_REQUIRE(code[k] >= 0 && code[k] <= 4, "csmae_recon_panel: panel%d = %d is no panel code (0 x, 1 xm, 2 y, 3 ym, 4 xm_ym)", k, code[k]);
    codes |= (unsigned)code[k] << (4 * k);
  }
  CSMAE_REQUIRE(gap >= 0, "csmae_recon_panel: gap = %d must not be negative", gap);
  const long long W = (long long)n_panels * S + (long long)(n_panels - 1) * gap, B = 3 * W * S;
  CSMAE_REQUIRE((long long)S + gap <= 0x7fffffffLL && B <= 0x7fffffffLL, "csmae_recon_panel: a sheet of S = %d, n_panels = %d, gap = %d is beyond 2^31 bytes per image", S,
                n_panels, gap);
  const long long bpi = (B + 3 + 1023) / 1024, blocks = N * bpi;   // (+ 3: the first dword may start 3 bytes before the sheet)
  CSMAE_REQUIRE(blocks <= 0x7fffffffLL, "csmae_recon_panel: N = %lld sheets of %lld bytes are beyond the grid", N, B);
  RpGeom g;
  g.C = C; g.S = S; g.p = p; g.G = (int)G; g.PW = S + gap; g.W3 = (int)(3 * W); g.B = (unsigned)B; g.bpi = (unsigned)bpi;
  g.br = band_r; g.bg = band_g; g.bb = band_b; g.codes = codes;
  hipStream_t st = (hipStream_t)stream;
  if (pred_dtype == CSMAE_F32)
    hipLaunchKernelGGL(recon_panel_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, g, img, (const float*)pred, ldp, img_stride, mask, mean, std, out);
  else
    hipLaunchKernelGGL(recon_panel_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, g, img, (const bf16_t*)pred, ldp, img_stride, mask, mean, std, out);
  return csmae_check_launch("csmae_recon_panel");
}
