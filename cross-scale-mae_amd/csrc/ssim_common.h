// The separable 11-tap gaussian FIR of the ssim kernels (ssim.hip: the loss family and its backward; recon_eval.hip: per-image evaluation
// scores): the window of pytorch-msssim 0.2.1, the stabilisers for data_range 1, staging of a tile of two planes into LDS and the two passes.
#pragma once
#include "common.h"

#define SSIM_WIN 11
#define SSIM_R (SSIM_WIN - 1)
#define SSIM_TILE 32
struct SsimWin { float w[SSIM_WIN]; };
static SsimWin ssim_window() {  // pytorch-msssim `_fspecial_gauss_1d(11, 1.5)` in fp32
  SsimWin w; float s = 0.f;
  for (int i = 0; i < SSIM_WIN; ++i) { float c = (float)(i - SSIM_WIN / 2); w.w[i] = expf(-(c * c) / (2.f * 1.5f * 1.5f)); s += w.w[i]; }
  for (int i = 0; i < SSIM_WIN; ++i) w.w[i] /= s;
  return w;
}

#define SSIM_C1 1.0e-4f   // (0.01 * data_range)^2, data_range = 1
#define SSIM_C2 9.0e-4f   // (0.03 * data_range)^2
// 11-tap FIR over a register window: four consecutive outputs from fourteen consecutive inputs (each LDS value is read once per
// four outputs instead of once per tap).  Every element is a PAIR of independent signals (two adjacent columns in the passes along
// H, two adjacent rows in the passes along W), so that the multiply-adds are gfx950's packed fp32 instructions: these kernels are
// bound by VALU issue, not by HBM or LDS.
__device__ __forceinline__ void fir4(const SsimWin& w, const f2_t (&in)[4 + SSIM_R], f2_t (&out)[4]) {
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    f2_t a = in[o] * w.w[0];
#pragma unroll
    for (int k = 1; k < SSIM_WIN; ++k) a += in[o + k] * w.w[k];
    out[o] = a;
  }
}
__device__ __forceinline__ f2_t rcp2(f2_t v) { return f2_t{__builtin_amdgcn_rcpf(v[0]), __builtin_amdgcn_rcpf(v[1])}; }
// stage a (rows x 2*pairs) window of two planes into LDS (zero outside the plane); 8-byte loads when the plane rows allow it
template <int ROWS, int PAIRS, int STRIDE>
__device__ __forceinline__ void ssim_stage(const float* __restrict__ px, const float* __restrict__ py, int H, int gy0, int gx0, float* sx, float* sy) {
  const bool vec = (H & 1) == 0;   // gx0 is even: a pair is 8-byte aligned and lies inside or outside the plane as a whole
  for (int i = threadIdx.x; i < ROWS * PAIRS; i += 256) {
    const int r = i / PAIRS, cp = i - r * PAIRS, gy = gy0 + r, gx = gx0 + 2 * cp;
    f2_t x = {0.f, 0.f}, y = {0.f, 0.f};
    if (gy >= 0 && gy < H) {
      if (vec) { if (gx >= 0 && gx < H) { x = *reinterpret_cast<const f2_t*>(px + (long long)gy * H + gx); y = *reinterpret_cast<const f2_t*>(py + (long long)gy * H + gx); } }
      else {
        if (gx >= 0 && gx < H) { x[0] = px[(long long)gy * H + gx]; y[0] = py[(long long)gy * H + gx]; }
        if (gx + 1 >= 0 && gx + 1 < H) { x[1] = px[(long long)gy * H + gx + 1]; y[1] = py[(long long)gy * H + gx + 1]; }
      }
    }
    *reinterpret_cast<f2_t*>(sx + r * STRIDE + 2 * cp) = x;
    *reinterpret_cast<f2_t*>(sy + r * STRIDE + 2 * cp) = y;
  }
}
// pass along H over staged planes: for NRG groups of four rows and NCP column pairs, the five filtered quantities
// (x, y, x^2, y^2, xy) -> V[m][row][col]
template <int NRG, int NCP, int SIN, int SOUT, int VROWS>
__device__ __forceinline__ void ssim_pass_h(const SsimWin& win, const float* sx, const float* sy, float* V) {
  for (int i = threadIdx.x; i < NRG * NCP; i += 256) {
    const int rg = i / NCP, cp = i - rg * NCP;
    f2_t x[4 + SSIM_R], y[4 + SSIM_R], t[4 + SSIM_R], o[4];
#pragma unroll
    for (int k = 0; k < 4 + SSIM_R; ++k) {
      x[k] = *reinterpret_cast<const f2_t*>(sx + (rg * 4 + k) * SIN + 2 * cp);
      y[k] = *reinterpret_cast<const f2_t*>(sy + (rg * 4 + k) * SIN + 2 * cp);
    }
    auto put = [&](int m) {
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<f2_t*>(V + (m * VROWS + rg * 4 + j) * SOUT + 2 * cp) = o[j];
    };
    fir4(win, x, o); put(0);
    fir4(win, y, o); put(1);
#pragma unroll
    for (int k = 0; k < 4 + SSIM_R; ++k) t[k] = x[k] * x[k];
    fir4(win, t, o); put(2);
#pragma unroll
    for (int k = 0; k < 4 + SSIM_R; ++k) t[k] = y[k] * y[k];
    fir4(win, t, o); put(3);
#pragma unroll
    for (int k = 0; k < 4 + SSIM_R; ++k) t[k] = x[k] * y[k];
    fir4(win, t, o); put(4);
  }
}
// pass along W for one (row pair rp, column group c0): NM maps of V -> f[m][4] (element = the two rows)
template <int NM, int SV, int VROWS>
__device__ __forceinline__ void ssim_pass_w(const SsimWin& win, const float* V, int rp, int c0, f2_t (&f)[NM][4]) {
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    f2_t in[4 + SSIM_R];
    const float* v0 = V + (m * VROWS + 2 * rp) * SV + c0;
#pragma unroll
    for (int k = 0; k < 4 + SSIM_R; ++k) in[k] = f2_t{v0[k], v0[SV + k]};
    fir4(win, in, f[m]);
  }
}
