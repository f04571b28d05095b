// Overlay sheets, the argmax map and per-image counts of the linear segmentation probe, for a whole batch, in one launch (util/seg_viz.py
// segmentation_panels, main_segprobe.py --panel_dir / --pred_dir / --per_image).  From the operands the loss kernel scores: the patch logits
// [N, G, G, K] are upsampled bilinearly in registers (csrc/seg_common.h: seg_ce's expression and tie rule), never to memory.
//   out   uint8 [N][S][W][3], W = n_panes S + (n_panes - 1) gap: per image one RGB row of panes, `gap` white pixels between neighbours
//   pred  uint8 [N][S][S] (nullable): the argmax class of every pixel
//   stats int32 [N][K][3] (nullable): per image and class (intersection, label area, prediction area) over the pixels whose label is < K
// With b the displayed image's byte (recon_panel's rule: (int) min(max(255 (img std + mean), 0), 255)), arg the argmax class, `valid` = label < K and
// blend(b, c) = (b (256 - a8) + c a8 + 128) >> 8 in integers, a pane shows by its code
//   0 image: b    1 gt: palette[label] | ignore_rgb    2 pred: palette[arg]    3 gt_over: blend(b, palette[label] | ignore_rgb)
//   4 pred_over: blend(b, palette[arg])    5 errors: valid ? (arg != label ? blend(b, red) : b) : blend(b, ignore_rgb)
//
// A workgroup owns a band of R consecutive pixel rows of ONE image (R S about 2048 pixels).
//   Phase 1: a thread per pixel forms arg once and leaves it, with the label, in LDS; pred goes out; the counts go to an LDS histogram of 3 K ints.
//   Phase 2: the band's bytes are ONE flat range of R 3 W bytes of the sheet, stored the way recon_panel.hip stores an image's: lane j owns the j-th
//   ALIGNED dword that touches the range, finds (row, column, channel) of its first byte with two divisions and walks the other three by
//   increments.  Only the first and the last dword of a band can hang over its ends: their inside bytes leave as byte stores, so the neighbouring
//   band's bytes (or the memory around the buffer) are never touched and every byte is written exactly once.
// The histogram is flushed with one integer atomic per non-zero entry onto stats, which the library clears on the stream first: integer sums, so two
// runs give the same counts.  Plain fp32, no MFMA: the kernel is bound by the bytes it writes and by the K-long argmax walk over cached logits.
#include "common.h"
#include "seg_common.h"

#define SP_KMAX 64
#define SP_BAND_PIXELS 2048

struct SpGeom {
  int C, S, p, G, K, R, PW, W3;   // R: pixel rows of a band; PW = S + gap: a pane and the gap behind it; W3 = 3 W: bytes of a sheet row
  unsigned B, bpi;                // bytes of one image's sheet; bands (workgroups) per image
  int br, bg, bb;                 // the channels shown as red, green, blue
  unsigned codes;                 // pane k's code in bits [4 k, 4 k + 4)
  unsigned ign;                   // ignore_rgb: r | g << 8 | b << 16
  int a8;
};

// truncating, clamped, defined for every input: a NaN fails the first comparison (0), +inf the second (255)
__device__ __forceinline__ unsigned sp_to_byte(float v) {
  const float t = v * 255.f;
  return t >= 0.f ? (t < 255.f ? (unsigned)(int)t : 255u) : 0u;
}
__device__ __forceinline__ unsigned sp_blend(unsigned b, unsigned c, int a8) { return (b * (unsigned)(256 - a8) + c * (unsigned)a8 + 128u) >> 8; }

// the byte at (band row yr, sheet column col, channel ch)
__device__ __forceinline__ unsigned sp_value(const SpGeom& g, const float* __restrict__ pi, const float* __restrict__ mean, const float* __restrict__ std,
                                             const unsigned char* s_arg, const unsigned char* s_lab, const unsigned char* s_pal, unsigned y0, unsigned yr,
                                             unsigned col, unsigned ch) {
  const unsigned k = col / (unsigned)g.PW, x = col - k * g.PW;
  if (x >= (unsigned)g.S) return 255u;   // the gap
  const unsigned code = (g.codes >> (4 * k)) & 15u;
  const unsigned j = yr * g.S + x;
  const unsigned arg = s_arg[j], label = s_lab[j];
  const bool valid = label < (unsigned)g.K;
  unsigned b = 0;
  if (code != 1 && code != 2) {
    const int c = ch == 0 ? g.br : ch == 1 ? g.bg : g.bb;
    b = sp_to_byte(pi[((long long)c * g.S + (y0 + yr)) * g.S + x] * std[c] + mean[c]);
  }
  const unsigned ign = (g.ign >> (8 * ch)) & 255u;
  switch (code) {
    case 0: return b;
    case 1: return valid ? s_pal[label * 3 + ch] : ign;
    case 2: return s_pal[arg * 3 + ch];
    case 3: return sp_blend(b, valid ? s_pal[label * 3 + ch] : ign, g.a8);
    case 4: return sp_blend(b, s_pal[arg * 3 + ch], g.a8);
    default: return valid ? (arg != label ? sp_blend(b, ch == 0 ? 255u : 0u, g.a8) : b) : sp_blend(b, ign, g.a8);
  }
}

__global__ __launch_bounds__(256) void seg_panel_kernel(SpGeom g, const float* __restrict__ img, const float* __restrict__ mean, const float* __restrict__ std,
                                                        const float* __restrict__ pl, const unsigned char* __restrict__ lab, const unsigned char* __restrict__ palette,
                                                        unsigned char* __restrict__ out, unsigned char* __restrict__ pred, int* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sp_smem[];
  int* hist = reinterpret_cast<int*>(sp_smem);              // 3 SP_KMAX ints
  unsigned char* s_pal = sp_smem + 3 * SP_KMAX * 4;          // 3 SP_KMAX bytes
  unsigned char* s_arg = s_pal + 3 * SP_KMAX;                // R S bytes
  unsigned char* s_lab = s_arg + g.R * g.S;                  // R S bytes
  const long long n = blockIdx.x / g.bpi;
  const unsigned band = (unsigned)(blockIdx.x - n * g.bpi);
  const unsigned y0 = band * g.R, rows = min((unsigned)g.R, (unsigned)g.S - y0), npx = rows * g.S;
  for (int i = threadIdx.x; i < 3 * g.K; i += 256) { hist[i] = 0; s_pal[i] = palette[i]; }
  __syncthreads();
  // ---- phase 1: the argmax of every pixel of the band
  const float* pln = pl + n * g.G * g.G * g.K;
  const long long pix0 = (n * g.S + y0) * g.S;   // the band's first pixel in [N][S][S]
  for (unsigned j = threadIdx.x; j < npx; j += 256) {
    const unsigned yr = j / (unsigned)g.S, x = j - yr * g.S;
    const int label = lab != nullptr ? (int)lab[pix0 + j] : CSMAE_SEG_IGNORE;
    const SegPixel px = seg_pixel(pln, g.G, g.K, seg_axis((int)(y0 + yr), g.p, g.G), seg_axis((int)x, g.p, g.G));
    float m = -INFINITY;
    int arg = 0;
    for (int k = 0; k < g.K; ++k) {
      const float z = px.z(k);
      if (z > m) { m = z; arg = k; }   // (strict: the lowest index wins ties, as in seg_ce)
    }
    s_arg[j] = (unsigned char)arg;
    s_lab[j] = (unsigned char)label;
    if (pred != nullptr) pred[pix0 + j] = (unsigned char)arg;
    if (stats != nullptr && label < g.K) {
      atomicAdd(&hist[3 * label + 1], 1);
      atomicAdd(&hist[3 * arg + 2], 1);
      if (arg == label) atomicAdd(&hist[3 * label], 1);
    }
  }
  __syncthreads();
  if (stats != nullptr) {
    int* ps = stats + n * 3 * g.K;
    for (int i = threadIdx.x; i < 3 * g.K; i += 256) {
      const int c = hist[i];
      if (c != 0) atomicAdd(ps + i, c);
    }
  }
  // ---- phase 2: the band's bytes of the sheet
  const unsigned len = rows * (unsigned)g.W3;
  unsigned char* po = out + n * (long long)g.B + (long long)y0 * g.W3;
  const float* pi = img + n * g.C * g.S * g.S;
  const int mis = (int)((uintptr_t)po & 3);
  for (unsigned jd = threadIdx.x;; jd += 256) {
    const long long o0 = 4ll * jd - mis;   // offset in the band of the first byte of aligned dword jd: -3 .. len + 2
    if (o0 >= (long long)len) break;
    const unsigned first = o0 < 0 ? 0u : (unsigned)o0;
    unsigned yr = first / (unsigned)g.W3, r = first - yr * g.W3, col = r / 3u, ch = r - col * 3u;
    unsigned word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const long long o = o0 + b;
      if (o < 0 || o >= (long long)len) continue;
      word |= sp_value(g, pi, mean, std, s_arg, s_lab, s_pal, y0, yr, col, ch) << (8 * b);
      if (++ch == 3u) { ch = 0; ++col; }
      if (++r == (unsigned)g.W3) { r = 0; col = 0; ++yr; }
    }
    if (o0 >= 0 && o0 + 4 <= (long long)len) {
      *reinterpret_cast<unsigned*>(po + o0) = word;
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (o0 + b >= 0 && o0 + b < (long long)len) po[o0 + b] = (unsigned char)(word >> (8 * b));
    }
  }
}

extern "C" int csmae_segpanel(long long N, int C, int S, int G, int p, int K, const float* img, const float* mean, const float* std, int band_r, int band_g,
                               int band_b, const float* pl, const unsigned char* labels, const unsigned char* palette, int ignore_r, int ignore_g, int ignore_b,
                               int a8, int pane0, int pane1, int pane2, int pane3, int pane4, int pane5, int n_panes, int gap, unsigned char* out,
                               unsigned char* pred, int* stats, void* stream) {
  CSMAE_REQUIRE(img && mean && std && pl && palette && out, "csmae_segpanel: null argument (img, mean, std, pl, palette or out)");
  CSMAE_REQUIRE(N > 0 && C >= 1, "csmae_segpanel: N = %lld, C = %d must be positive", N, C);
  CSMAE_REQUIRE(K >= 2 && K <= SP_KMAX, "csmae_segpanel: K = %d classes; the kernel holds 2 .. %d", K, SP_KMAX);
  CSMAE_REQUIRE(p == 4 || p == 8 || p == 14 || p == 16, "csmae_segpanel: patch size %d; the kernel takes 4, 8, 14 or 16", p);
  CSMAE_REQUIRE(G >= 1 && G <= 4096, "csmae_segpanel: a grid of %d cells per side; the kernel takes 1 .. 4096", G);
  CSMAE_REQUIRE(S == G * p, "csmae_segpanel: an image of %d x %d pixels does not fit %d x %d cells of %d pixels", S, S, G, G, p);
  CSMAE_REQUIRE(n_panes >= 1 && n_panes <= 6, "csmae_segpanel: n_panes = %d must lie in [1, 6]", n_panes);
  const int code[6] = {pane0, pane1, pane2, pane3, pane4, pane5};
  unsigned codes = 0;
  for (int k = 0; k < n_panes; ++k) {
    CSMAE_REQUIRE(code[k] >= 0 && code[k] <= 5, "csmae_segpanel: pane%d = %d is no pane code (0 image, 1 gt, 2 pred, 3 gt_over, 4 pred_over, 5 errors)", k, code[k]);
    CSMAE_REQUIRE(labels || (code[k] != 1 && code[k] != 3 && code[k] != 5), "csmae_segpanel: pane%d = %d shows the labels, which are null", k, code[k]);
    codes |= (unsigned)code[k] << (4 * k);
  }
  CSMAE_REQUIRE(labels || !stats, "csmae_segpanel: stats count against the labels, which are null");
  CSMAE_REQUIRE(band_r >= 0 && band_r < C && band_g >= 0 && band_g < C && band_b >= 0 && band_b < C,
                "csmae_segpanel: band_r, band_g, band_b = %d, %d, %d must lie in [0, C = %d)", band_r, band_g, band_b, C);
  CSMAE_REQUIRE(gap >= 0, "csmae_segpanel: gap = %d must not be negative", gap);
  CSMAE_REQUIRE(a8 >= 0 && a8 <= 256, "csmae_segpanel: a8 = %d must lie in [0, 256]", a8);
  CSMAE_REQUIRE((ignore_r | ignore_g | ignore_b) >= 0 && (ignore_r | ignore_g | ignore_b) <= 255, "csmae_segpanel: ignore_rgb = %d, %d, %d must be bytes", ignore_r,
                ignore_g, ignore_b);
  const long long W = (long long)n_panes * S + (long long)(n_panes - 1) * gap, B = 3 * W * S;
  CSMAE_REQUIRE((long long)S + gap <= 0x7fffffffLL && W <= 0x7fffffffLL / 3 && N <= 0x7fffffffLL && B <= 0x7fffffffLL / N,
                "csmae_segpanel: N = %lld sheets of S = %d, n_panes = %d, gap = %d are 2^31 bytes or more", N, S, n_panes, gap);
  const int R = max(1, min(S, SP_BAND_PIXELS / S));
  const long long bpi = (S + R - 1) / R, blocks = N * bpi;
  CSMAE_REQUIRE(blocks <= 0x7fffffffLL, "csmae_segpanel: N = %lld images of %lld bands are beyond the grid", N, bpi);
  const size_t lds = 3 * SP_KMAX * 4 + 3 * SP_KMAX + 2 * (size_t)R * S;   // (R S <= max(2048, S), S < 2^15.5 by the byte bound: under 64 KiB)
  CSMAE_REQUIRE(lds <= 65536, "csmae_segpanel: a pixel row of S = %d does not fit the workgroup's memory", S);
  SpGeom g;
  g.C = C; g.S = S; g.p = p; g.G = G; g.K = K; g.R = R; g.PW = S + gap; g.W3 = (int)(3 * W); g.B = (unsigned)B; g.bpi = (unsigned)bpi;
  g.br = band_r; g.bg = band_g; g.bb = band_b; g.codes = codes;
  g.ign = (unsigned)ignore_r | (unsigned)ignore_g << 8 | (unsigned)ignore_b << 16;
  g.a8 = a8;
  hipStream_t st = (hipStream_t)stream;
  if (stats != nullptr) {
    const hipError_t e = hipMemsetAsync(stats, 0, (size_t)N * K * 3 * sizeof(int), st);
    CSMAE_REQUIRE(e == hipSuccess, "csmae_segpanel: clearing stats failed: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(seg_panel_kernel, dim3((unsigned)blocks), dim3(256), lds, st, g, img, mean, std, pl, labels, palette, out, pred, stats);
  return csmae_check_launch("csmae_segpanel");
}
