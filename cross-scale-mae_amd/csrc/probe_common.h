// Token pooling shared by the probe's forward (linprobe.hip) and the fine-tune head's backward (finetune.hip): one workgroup per sample; a
// thread owns V consecutive columns (16 bytes of the row) and every `lanes`-th token, the token lanes are folded through LDS, the row
// statistics through block_sum (two passes: mean, then centred squares).
#pragma once
#include "common.h"

#define POOL_THREADS 1024
#define POOL_LDS 8192   // floats: lanes * D <= POOL_THREADS * V <= 8192
template <typename T, int V> __device__ __forceinline__ void pool_ld(const T* p, float* v);
template <> __device__ __forceinline__ void pool_ld<float, 4>(const float* p, float* v) {
  const f4_t a = *reinterpret_cast<const f4_t*>(p);
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
}
template <> __device__ __forceinline__ void pool_ld<bf16_t, 4>(const bf16_t* p, float* v) {
  const f4_t a = ld4<bf16_t>(p);
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
}
template <> __device__ __forceinline__ void pool_ld<bf16_t, 8>(const bf16_t* p, float* v) {
  const uint4 u = *reinterpret_cast<const uint4*>(p);
  v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
  v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
  v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u);
  v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
}
// Mean of tokens [t0, t1) of one sample `xs` [T, D] -> acc[0 .. D) (LDS, POOL_LDS floats), and the LayerNorm statistics of that row.  Every thread
// of the workgroup calls it; on return thread d owns columns d, d + blockDim.x, ... of acc.
template <typename T, int V>
__device__ __forceinline__ void pool_row_stats(int D, int t0, int t1, const T* __restrict__ xs, float eps, float* acc, float* red /* 17 floats */, float& mean,
                                               float& rstd) {
  const int groups = D / V;                 // column groups of a row (host: D % V == 0, groups <= POOL_THREADS)
  const int lanes = min(POOL_THREADS / groups, t1 - t0);   // token lanes that have work (>= 1)
  const int cg = threadIdx.x % groups, tl = threadIdx.x / groups;
  if (tl < lanes) {
    float s[V];
#pragma unroll
    for (int k = 0; k < V; ++k) s[k] = 0.f;
    for (int t = t0 + tl; t < t1; t += lanes) {
      float v[V];
      pool_ld<T, V>(xs + (long long)t * D + cg * V, v);
#pragma unroll
      for (int k = 0; k < V; ++k) s[k] += v[k];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) acc[tl * D + cg * V + k] = s[k];
  }
  __syncthreads();
  // fold the token lanes (fixed order) and take the mean: thread d owns column d, d + blockDim.x, ...
  const float cnt = (float)(t1 - t0);
  float part = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float s = acc[d];
    for (int l = 1; l < lanes; ++l) s += acc[l * D + d];
    s = s / cnt;
    acc[d] = s;   // (row 0 of acc is only read by its owner before this write)
    part += s;
  }
  mean = block_sum(part, red) / (float)D;
  part = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) { const float c = acc[d] - mean; part += c * c; }
  rstd = rsqrtf(block_sum(part, red) / (float)D + eps);
}
