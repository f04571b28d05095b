// Multispectral input step: 13-band Sentinel-2 (EuroSAT) tiles, uint16 in raw reflectance units, through the transform chain the reference
// applies to them (util/datasets.py:489-564; Dataset_eurosat inherits BaseDataset.build_transform, :108-158):
//   masked bands := the band's mean -> ToTensor (no / 255 for a float array) -> Normalize(mean, std) ->
//   train: horizontal / vertical flip, RandomResizedCrop(S, scale (0.25, 1), bicubic, antialias)
//   eval:  Resize(int(S / crop_pct), bicubic, antialias), CenterCrop(S)
//   -> the dropped bands are removed.
// The geometry, the RNG order and the resampling rule are those of augment_u8_kernel / eval_u8_kernel (csrc/tokens.hip), and `meta` has the same
// meaning; what differs is the source type, the band count and the band plan.  The helpers below restate the tap rule of tokens.hip (the u8
// kernels keep their own copy untouched; tests/test_ms_input_cpu.py holds MS_MAX_TAPS to AUG_MAX_TAPS).
#include "common.h"

#define MS_MAX_BANDS 13
#define MS_MAX_TAPS 96            // taps of one axis a window may hold: AUG_MAX_TAPS of tokens.hip, EVAL_MAX_TAPS of util/gpu_input.py
#define MS_MAX_ROW_FLOATS 12288   // one resampled source row [Wmax][Cin] fp32 in LDS: 48 KiB (Wmax <= 945 at 13 bands)

namespace {
// ATen's separable anti-aliased bicubic (a = -0.5): output o of an axis resampled at `scale = in / out` has the centre c = scale * (o + 0.5), the
// window [int(c - sup + 0.5), int(c + sup + 0.5)) clipped to the input with sup = 2 max(scale, 1), and tap k of a window that starts at `lo` weighs
// cubic((k + lo - c + 0.5) / max(scale, 1)); the weights are renormalised over the clipped window.
__device__ __forceinline__ float ms_cubic(float x) {
  x = fabsf(x);
  const float a = -0.5f;
  if (x < 1.f) return ((a + 2.f) * x - (a + 3.f)) * x * x + 1.f;
  if (x < 2.f) return (((x - 5.f) * x + 8.f) * x - 4.f) * a;
  return 0.f;
}
__device__ __forceinline__ void ms_support(float scale, float& sup, float& inv) {
  sup = scale >= 1.f ? 2.f * scale : 2.f;
  inv = scale >= 1.f ? 1.f / scale : 1.f;
}
__device__ __forceinline__ float ms_weight(int k, int lo, float c, float inv) { return ms_cubic((k + lo - c + 0.5f) * inv); }
// The window of output o as (first tap, tap count, centre relative to `base`): tap k weighs ms_weight(k, lo - base, c, inv).
//   train (box -> S): the centre scale * (o + 0.5) in fp32, base 0 — augment_u8_kernel's arithmetic;
//   eval (in -> out): the centre in * (2 o + 1) / (2 out) split into its integer part (base) and a fraction in [0, 1), so that an elongated
//   image keeps the fraction's precision — eval_u8_kernel's arithmetic.  The host refuses in * 2 out >= 2^31 and more than MS_MAX_TAPS taps.
template <bool EVAL>
__device__ __forceinline__ void ms_window(int in, int out, int o, float sup, int& lo, int& n, int& base, float& c) {
  int hi;
  if (EVAL) {
    const unsigned num = (unsigned)in * (unsigned)(2 * o + 1), den = 2u * (unsigned)out;
    const unsigned q = num / den;
    base = (int)q;
    c = (float)(num - q * den) / (float)den;
    lo = base + (int)floorf(c - sup + 0.5f);
    hi = base + (int)floorf(c + sup + 0.5f);
  } else {
    base = 0;
    c = ((float)in / (float)out) * (o + 0.5f);
    lo = (int)(c - sup + 0.5f);
    hi = (int)(c + sup + 0.5f);
  }
  lo = lo < 0 ? 0 : lo;
  hi = hi > in ? in : hi;
  n = hi - lo;
  n = n > MS_MAX_TAPS ? MS_MAX_TAPS : (n < 0 ? 0 : n);   // (keeps wy[] and every read in bounds whatever meta holds)
}
__device__ __forceinline__ int ms_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The band plan by value: src[k] = source band of output channel k, bit 8 = masked; used = the source bands some unmasked output channel reads.
struct MsBands { int src[MS_MAX_BANDS]; unsigned used; };

// One workgroup per (image, output row), two passes through LDS.
//   1. vertical: the lanes walk the contiguous (x, c) run of the source rows under the window — element e of the run is column x0 + e / Cin, band
//      e % Cin, so a wave reads 128 consecutive bytes per tap — and leave sum_a wy[a] * row_a[e] in row[e].  A band no output channel needs
//      (dropped, or masked: its value is the mean whatever the tile holds) is not loaded; its slot holds 0.
//   2. horizontal: one lane per output column gathers its taps from row[] for every output channel (neighbouring lanes read the same or
//      neighbouring source columns, Cin floats apart) and stores channel by channel, consecutive lanes to consecutive addresses.
// Normalisation comes last, (v - mean) * inv_std on the resampled raw value: it is linear and the weights sum to one.
template <bool EVAL>
__global__ __launch_bounds__(256) void ms_u16_kernel(int Cin, int Cout, int Hmax, int Wmax, int S, const unsigned short* __restrict__ src,
                                                     const int* __restrict__ meta, MsBands bands, const float* __restrict__ mean,
                                                     const float* __restrict__ inv_std, float* __restrict__ dst) {
  extern __shared__ float row[];   // [cols * Cin]
  __shared__ float wy[MS_MAX_TAPS];
  __shared__ int ylo_s, yn_s;
  const long long n = blockIdx.x;
  const int oy = blockIdx.y, tid = threadIdx.x;
  const int* mt = meta + n * 8;
  const int H = ms_clamp(mt[0], 1, Hmax), W = ms_clamp(mt[1], 1, Wmax);   // no read leaves the image's slot of src
  // rows: in_y source rows starting at y0 (of the flipped image for the training transform) -> out_y rows, of which this is row oy + top
  int y0, in_y, out_y, top, x0, in_x, out_x, left, hf = 0, vf = 0;
  if (EVAL) {
    y0 = 0; in_y = H; out_y = mt[2] < 1 ? 1 : mt[2]; top = mt[4];
    x0 = 0; in_x = W; out_x = mt[3] < 1 ? 1 : mt[3]; left = mt[5];
  } else {
    y0 = ms_clamp(mt[2], 0, H - 1); in_y = ms_clamp(mt[4], 1, H - y0); out_y = S; top = 0;
    const int bj = ms_clamp(mt[3], 0, W - 1);
    in_x = ms_clamp(mt[5], 1, W - bj); out_x = S; left = 0;
    hf = mt[6] != 0; vf = mt[7] != 0;
    x0 = hf ? W - bj - in_x : bj;   // the box's columns in the stored (un-flipped) image: [x0, x0 + in_x)
  }
  float supy, invy, supx, invx;
  ms_support((float)in_y / (float)out_y, supy, invy);
  ms_support((float)in_x / (float)out_x, supx, invx);
  if (tid == 0) {
    int lo, nn, base; float c;
    ms_window<EVAL>(in_y, out_y, oy + top, supy, lo, nn, base, c);
    float tot = 0.f;
    for (int k = 0; k < nn; ++k) { const float w = ms_weight(k, lo - base, c, invy); wy[k] = w; tot += w; }
    for (int k = 0; k < nn; ++k) wy[k] /= tot;
    ylo_s = lo; yn_s = nn;
  }
  __syncthreads();
  const int ylo = ylo_s, yn = yn_s;
  const unsigned short* img = src + n * (long long)Hmax * Wmax * Cin;
  const int run = in_x * Cin;
  for (int e = tid; e < run; e += blockDim.x) {
    float acc = 0.f;
    if ((bands.used >> (e % Cin)) & 1u) {
      for (int a = 0; a < yn; ++a) {
        int yy = y0 + ylo + a; yy = vf ? H - 1 - yy : yy;   // row of the flipped image -> row of the stored image
        acc = fmaf(wy[a], (float)img[((long long)yy * Wmax + x0) * Cin + e], acc);
      }
    }
    row[e] = acc;
  }
  __syncthreads();
  for (int ox = tid; ox < S; ox += blockDim.x) {
    int xlo, xn, base; float c;
    ms_window<EVAL>(in_x, out_x, ox + left, supx, xlo, xn, base, c);
    float acc[MS_MAX_BANDS];
#pragma unroll
    for (int k = 0; k < MS_MAX_BANDS; ++k) acc[k] = 0.f;
    float tot = 0.f;
    for (int b = 0; b < xn; ++b) {
      const float w = ms_weight(b, xlo - base, c, invx);
      tot += w;
      const int t = xlo + b;                                 // column of the (flipped) box -> column of the staged run
      const float* px = row + (hf ? in_x - 1 - t : t) * Cin;
#pragma unroll
      for (int k = 0; k < MS_MAX_BANDS; ++k) if (k < Cout) acc[k] = fmaf(w, px[bands.src[k] & 0xFF], acc[k]);
    }
    const float rt = 1.f / tot;
#pragma unroll
    for (int k = 0; k < MS_MAX_BANDS; ++k)
      if (k < Cout) dst[((n * Cout + k) * S + oy) * (long long)S + ox] = (bands.src[k] & 0x100) ? 0.f : (acc[k] * rt - mean[k]) * inv_std[k];
  }
}

int ms_launch(bool eval, const char* name, long long N, int Cin, int Cout, int Hmax, int Wmax, int S, const unsigned short* src, const int* meta,
              const int* band, const float* mean, const float* inv_std, float* dst, void* stream) {
  CSMAE_REQUIRE(src && meta && band && mean && inv_std && dst, "%s: null pointer", name);
  CSMAE_REQUIRE(N > 0 && N <= 0x7fffffffLL && Hmax > 0 && Wmax > 0 && S > 0 && S <= 65535, "%s: bad geometry N=%lld Hmax=%d Wmax=%d S=%d (S <= 65535)", name, N, Hmax, Wmax, S);
  CSMAE_REQUIRE(1 <= Cout && Cout <= Cin && Cin <= MS_MAX_BANDS, "%s: bad band counts Cin=%d Cout=%d (1 <= Cout <= Cin <= %d)", name, Cin, Cout, MS_MAX_BANDS);
  CSMAE_REQUIRE((long long)Wmax * Cin <= MS_MAX_ROW_FLOATS, "%s: a source row of Wmax=%d x Cin=%d values does not fit the %d floats of LDS the kernel keeps", name, Wmax, Cin,
                MS_MAX_ROW_FLOATS);
  MsBands b = {};
  for (int k = 0; k < Cout; ++k) {
    CSMAE_REQUIRE((band[k] & ~0x1FF) == 0 && (band[k] & 0xFF) < Cin, "%s: band[%d] = %d names no source band below Cin=%d (bit 8 = masked)", name, k, band[k], Cin);
    b.src[k] = band[k];
    if (!(band[k] & 0x100)) b.used |= 1u << (band[k] & 0xFF);
  }
  const dim3 grid((unsigned)N, (unsigned)S);
  const size_t lds = (size_t)Wmax * Cin * sizeof(float);
  if (eval) hipLaunchKernelGGL((ms_u16_kernel<true>), grid, dim3(256), lds, (hipStream_t)stream, Cin, Cout, Hmax, Wmax, S, src, meta, b, mean, inv_std, dst);
  else hipLaunchKernelGGL((ms_u16_kernel<false>), grid, dim3(256), lds, (hipStream_t)stream, Cin, Cout, Hmax, Wmax, S, src, meta, b, mean, inv_std, dst);
  return csmae_check_launch(name);
}
}  // namespace

extern "C" int csmae_augment_u16(long long N, int Cin, int Cout, int Hmax, int Wmax, int S, const unsigned short* src, const int* meta, const int* band,
                                 const float* mean, const float* inv_std, float* dst, void* stream) {
  return ms_launch(false, "csmae_augment_u16", N, Cin, Cout, Hmax, Wmax, S, src, meta, band, mean, inv_std, dst, stream);
}
extern "C" int csmae_eval_u16(long long N, int Cin, int Cout, int Hmax, int Wmax, int S, const unsigned short* src, const int* meta, const int* band,
                              const float* mean, const float* inv_std, float* dst, void* stream) {
  return ms_launch(true, "csmae_eval_u16", N, Cin, Cout, Hmax, Wmax, S, src, meta, band, mean, inv_std, dst, stream);
}
