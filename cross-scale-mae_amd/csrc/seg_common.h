// What the dense-prediction kernels share (csrc/segment.hip: the loss, its gradient; csrc/seg_panel.hip: the overlay sheets): one pixel's view of the
// patch logits under bilinear upsampling.  The upsampled logit is the same expression wherever it is formed, so the argmax a picture shows is the
// argmax the loss kernel scored.
#pragma once
#include "common.h"

// ---- bilinear upsampling of the patch logits, torch.nn.functional.interpolate(mode="bilinear", align_corners=False): output position i of an axis
// reads source coordinate max((i + 0.5) / p - 0.5, 0) = max(2 i + 1 - p, 0) / (2 p) — formed in integers, so the cell index is exact and the
// fraction takes one rounding; the second neighbour is clamped to G - 1.
struct SegAxis { int i0, i1; float f; };
__device__ __forceinline__ SegAxis seg_axis(int i, int p, int G) {
  const int t = max(2 * i + 1 - p, 0), q = t / (2 * p);   // q <= G - 1 for i < G p
  SegAxis a;
  a.i0 = q;
  a.i1 = min(q + 1, G - 1);
  a.f = (float)(t - q * 2 * p) / (float)(2 * p);
  return a;
}
// One pixel's view of the logits: the four neighbouring cells' rows and the weights of the two axes.  z(k) is the upsampled logit of class k, the
// same expression wherever it is formed: hy0 (hx0 a + hx1 b) + hy1 (hx0 c + hx1 d).
struct SegPixel {
  const float *a, *b, *c, *d;
  float hx0, hx1, hy0, hy1;
  __device__ __forceinline__ float z(int k) const { return hy0 * (hx0 * a[k] + hx1 * b[k]) + hy1 * (hx0 * c[k] + hx1 * d[k]); }
};
__device__ __forceinline__ SegPixel seg_pixel(const float* __restrict__ pln /* the image's [G, G, K] logits */, int G, int K, const SegAxis& ay, const SegAxis& ax) {
  SegPixel s;
  s.a = pln + ((long long)ay.i0 * G + ax.i0) * K;
  s.b = pln + ((long long)ay.i0 * G + ax.i1) * K;
  s.c = pln + ((long long)ay.i1 * G + ax.i0) * K;
  s.d = pln + ((long long)ay.i1 * G + ax.i1) * K;
  s.hx1 = ax.f; s.hx0 = 1.f - ax.f;
  s.hy1 = ay.f; s.hy0 = 1.f - ay.f;
  return s;
}
