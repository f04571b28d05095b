// What the loss heads share (loss.hip: reconstruction, pair, NT-Xent, finalize; ssim.hip: the ssim family): the per-element loss kinds, the
// patchify-on-the-fly geometry, the wave-per-patch prologue and the processed target.
#pragma once
#include "common.h"

// the per-element loss kinds of include/csmae.h (enum csmae_loss) under the short names the kernels use
constexpr int LOSS_MSE = CSMAE_LOSS_MSE, LOSS_L2 = CSMAE_LOSS_L2, LOSS_MAE = CSMAE_LOSS_MAE, LOSS_L1 = CSMAE_LOSS_L1, LOSS_BCE = CSMAE_LOSS_BCE;
constexpr int LOSS_NONE = 5;  // no per-patch term (pure ssim / ms_ssim): the gradient is the ssim family's `extra` alone

__device__ __forceinline__ float elem_loss(int kind, float pred, float t) {
  if (kind == LOSS_MSE || kind == LOSS_L2) { float d = pred - t; return d * d; }
  if (kind == LOSS_MAE || kind == LOSS_L1) return fabsf(pred - t);
  // bce with logits, torch's stable form: max(x,0) - x*t + log1p(exp(-|x|))
  return fmaxf(pred, 0.f) - pred * t + log1pf(expf(-fabsf(pred)));
}
__device__ __forceinline__ float elem_grad(int kind, float pred, float t) {  // d elem_loss / d pred
  if (kind == LOSS_MSE || kind == LOSS_L2) return 2.f * (pred - t);
  if (kind == LOSS_MAE || kind == LOSS_L1) { float d = pred - t; return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
  if (kind == LOSS_NONE) return 0.f;
  return 1.f / (1.f + expf(-pred)) - t;
}
__device__ __forceinline__ bool mean_over_last(int kind) { return kind == LOSS_MSE || kind == LOSS_MAE || kind == LOSS_BCE; }

// one wave per patch: target values of patch (n2, l); element e = (ph*p + pw)*C + c   (MAE_ViT_Shared.py:36-38 "nhwpqc")
struct PatchGeom { int N, C, S, p, L, G, P; unsigned mC, mp; };   // mC / mp: ceil(2^24 / C), ceil(2^24 / p) — n / d = (n * m) >> 24 for n * d < 2^24 (0: divide)
static inline PatchGeom make_geom(int N, int C, int S, int p) {
  PatchGeom g; g.N = N; g.C = C; g.S = S; g.p = p; g.G = S / p; g.L = g.G * g.G; g.P = p * p * C;
  const bool fast = (long long)g.P * (C > p ? C : p) < (1ll << 24);
  g.mC = fast ? (unsigned)(((1ull << 24) + C - 1) / C) : 0u; g.mp = fast ? (unsigned)(((1ull << 24) + p - 1) / p) : 0u;
  return g;
}
// the wave's patch, four waves per workgroup: pt of [B2 * L] = (sample n2 of both views, patch l); with cls = 1 the rows of [B2 * (L + 1)]
// (the backward kernels): pt is the row, l = -1 on a sample's cls row
struct PatchWave { int lane; long long pt, n2; int l, view; bool live; };
__device__ __forceinline__ PatchWave patch_wave(const PatchGeom& g, long long patches, int cls = 0) {
  PatchWave w; w.lane = threadIdx.x & 63; w.pt = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w.live = w.pt < patches;
  w.n2 = w.pt / (g.L + cls); w.l = (int)(w.pt - w.n2 * (g.L + cls)) - cls; w.view = (int)(w.n2 / g.N);
  return w;
}
__device__ __forceinline__ PatchWave patch_row_wave(const PatchGeom& g, long long rows) { return patch_wave(g, rows, 1); }
template <typename TP>
__device__ __forceinline__ const TP* pred_row(const PatchGeom& g, const TP* pred, long long ldp, const PatchWave& w) { return pred + (w.n2 * (g.L + 1) + 1 + w.l) * ldp; }
__device__ __forceinline__ const float* patch_img(const PatchGeom& g, const float* img0, const float* img1, long long n2) {
  int view = (int)(n2 / g.N);
  return (view ? img1 : img0) + (n2 - (long long)view * g.N) * g.C * g.S * g.S;
}
// element (c, ph, pw) of patch (gh, gw) in the planes [n2][C][S][S]
__device__ __forceinline__ long long patch_plane_offset(const PatchGeom& g, long long n2, int c, int gh, int ph, int gw, int pw) { return ((n2 * g.C + c) * g.S + gh * g.p + ph) * g.S + gw * g.p + pw; }
// element e of patch l of sample n2 -> its offset in the planes
__device__ __forceinline__ long long patch_elem_offset(const PatchGeom& g, long long n2, int l, int e) {
  const int gh = l / g.G, gw = l - gh * g.G;
  // (three integer divisions per element were most of this loop: exact multiply-shift instead when the operands allow it)
  const int r = g.mC ? (int)(((unsigned long long)(unsigned)e * g.mC) >> 24) : e / g.C, c = e - r * g.C;
  const int ph = g.mp ? (int)(((unsigned long long)(unsigned)r * g.mp) >> 24) : r / g.p, pw = r - ph * g.p;
  return patch_plane_offset(g, n2, c, gh, ph, gw, pw);
}
__device__ __forceinline__ float patch_elem(const PatchGeom& g, const float* img, int l, int e) { return img[patch_elem_offset(g, 0, l, e)]; }
// per-patch normalisation statistics (norm_pix_loss: unbiased variance, eps 1e-6 — MAE_ViT_Shared.py:106-109)
__device__ __forceinline__ void patch_stats(const PatchGeom& g, const float* img, int l, int lane, float& mu, float& rs) {
  float s = 0.f;
  for (int e = lane; e < g.P; e += 64) s += patch_elem(g, img, l, e);
  mu = wave_sum(s) / g.P;
  float q = 0.f;
  for (int e = lane; e < g.P; e += 64) { float d = patch_elem(g, img, l, e) - mu; q += d * d; }
  rs = rsqrtf(wave_sum(q) / (g.P - 1) + 1.0e-6f);
}
// the processed target: patch-normalised under norm_pix_loss, then (bce, the ssim family) min-max scaled over the view's whole tensor
struct TargetXform {
  float mu, rs, lo, sc; bool scaled;
  __device__ __forceinline__ float apply(float t) const { t = (t - mu) * rs; return scaled ? (t - lo) * sc : t; }
};
__device__ __forceinline__ TargetXform target_xform(const PatchGeom& g, const float* img, int l, int lane, int norm_pix, int kind,
                                                    const float* minmax /*[views][2]*/, int view) {
  TargetXform x{0.f, 1.f, 0.f, 1.f, kind == LOSS_BCE};
  if (norm_pix) patch_stats(g, img, l, lane, x.mu, x.rs);
  if (x.scaled) { x.lo = minmax[view * 2]; x.sc = 1.f / (minmax[view * 2 + 1] - x.lo + 1.0e-6f); }
  return x;
}

// launched from both translation units (no relocatable device code: a kernel is launched where it is defined, loss.hip)
void loss_launch_target_minmax(const PatchGeom& g, int norm_pix, long long patches, const float* img0, const float* img1, float* mm /*[patches][2]*/, hipStream_t st);
void loss_launch_minmax_reduce(long long per_view, int views, const float* mm, float* out /*[views][2]*/, hipStream_t st);
