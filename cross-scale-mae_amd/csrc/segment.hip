// Dense prediction on the frozen encoder (main_segprobe.py, models_seg.py): the two steps of a linear segmentation probe that the classification
// kernels (csrc/classify.hip: bn1d_fwd, head_linear_fwd / _bwd) do not cover.  All arithmetic is fp32; only the token stream may be bf16.  Small,
// latency- / cache-bound kernels (the logits of a ViT-B/16 batch of 64 are 0.8 MB; every operand is re-read from L1 / L2): plain fp32, no MFMA
// route, no floating-point atomics, fixed summation orders.  None has been profiled on its own.
//   seg_token_norm   residual stream [N, L + 1, D] -> LayerNorm of the L patch tokens, fp32 [N L, D] (the cls row is dropped)
//   seg_ce           patch logits [N, G, G, K] -> bilinear G x G -> S x S upsampling + mean cross-entropy against uint8 labels [N, S, S] with an ignore
//                    value, the valid count, the confusion matrix and the argmax map, without the upsampled logits ever reaching memory
//   seg_ce_bwd       the gradient of that loss w.r.t. the patch logits, as a gather over each cell's footprint
#include "common.h"
#include "seg_common.h"   // SegAxis / seg_axis, SegPixel / seg_pixel: the bilinear upsampling of the patch logits, shared with seg_panel.hip

// ---- LayerNorm of the patch tokens.  One wave per token, lanes across D; a workgroup is four waves.  Vector form: a lane holds up to SEG_LN_V4
// groups of 4 consecutive columns in registers (one read of the row); scalar form (any D, any alignment): three passes over the row, the
// second and third from cache.  Statistics in fp32: mean, then the centred squares.
#define SEG_LN_V4 8   // float4 groups per lane of the vector form: D <= 64 * 4 * 8
template <typename T>
__global__ __launch_bounds__(256) void seg_token_norm_v4_kernel(long long rows, int L, int D, const T* __restrict__ x, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float eps, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;   // (wave-uniform)
  const long long n = r / L;
  const T* src = x + (r + n + 1) * D;   // row n (L + 1) + 1 + l of the stream
  f4_t v[SEG_LN_V4];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < SEG_LN_V4; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = c < D ? ld4<T>(src + c) : f4_t{0.f, 0.f, 0.f, 0.f};
    s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  }
  const float mean = wave_sum(s) / (float)D;
  s = 0.f;
#pragma unroll
  for (int i = 0; i < SEG_LN_V4; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < D) {
      v[i] = v[i] - mean;
      s += (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
    }
  }
  const float rstd = rsqrtf(wave_sum(s) / (float)D + eps);
  float* dst = out + r * D;
#pragma unroll
  for (int i = 0; i < SEG_LN_V4; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < D) st4<float>(dst + c, v[i] * rstd * ld4<float>(gamma + c) + ld4<float>(beta + c));
  }
}
template <typename T>
__global__ __launch_bounds__(256) void seg_token_norm_kernel(long long rows, int L, int D, const T* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const long long n = r / L;
  const T* src = x + (r + n + 1) * D;
  float s = 0.f;
  for (int c = lane; c < D; c += 64) s += ld_as_f32<T>(src + c);
  const float mean = wave_sum(s) / (float)D;
  s = 0.f;
  for (int c = lane; c < D; c += 64) { const float d = ld_as_f32<T>(src + c) - mean; s += d * d; }
  const float rstd = rsqrtf(wave_sum(s) / (float)D + eps);
  float* dst = out + r * D;
  for (int c = lane; c < D; c += 64) dst[c] = (ld_as_f32<T>(src + c) - mean) * rstd * gamma[c] + beta[c];
}
extern "C" int csmae_seg_token_norm(int dtype, long long N, int T, int D, const void* x, const float* gamma, const float* beta, float eps, float* out,
                                    void* stream) {
  CSMAE_REQUIRE(N > 0 && T >= 2 && D >= 1 && x && gamma && beta && out, "csmae_seg_token_norm: null or empty argument (T = L + 1 >= 2: the cls row is dropped)");
  CSMAE_REQUIRE(dtype == CSMAE_F32 || dtype == CSMAE_BF16, "csmae_seg_token_norm: bad dtype %d", dtype);
  const int L = T - 1;
  const long long rows = N * L;
  CSMAE_REQUIRE(N <= 0x7fffffffLL && (rows + 3) / 4 <= 0x7fffffffLL, "csmae_seg_token_norm: N (T - 1) = %lld rows are beyond the grid", rows);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  const bool v4 = D % 4 == 0 && D <= 64 * 4 * SEG_LN_V4 && (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15) == 0;
#define STN(KERNEL, TT) hipLaunchKernelGGL((KERNEL<TT>), grid, block, 0, st, rows, L, D, (const TT*)x, gamma, beta, eps, out)
  if (v4) { if (dtype == CSMAE_F32) STN(seg_token_norm_v4_kernel, float); else STN(seg_token_norm_v4_kernel, bf16_t); }
  else { if (dtype == CSMAE_F32) STN(seg_token_norm_kernel, float); else STN(seg_token_norm_kernel, bf16_t); }
#undef STN
  return csmae_check_launch("csmae_seg_token_norm");
}

// maximum m of the pixel's K logits, its first position, s = sum_k exp(z_k - m), and the label's logit (0 when the label names no class); two walks
// over the classes, the logits formed twice from operands that sit in cache
__device__ __forceinline__ void seg_softmax_stats(const SegPixel& px, int K, int label, float& m, int& arg, float& s, float& zl) {
  m = -INFINITY; arg = 0; zl = 0.f;
  for (int k = 0; k < K; ++k) {
    const float z = px.z(k);
    if (z > m) { m = z; arg = k; }   // (strict: the lowest index wins ties)
    if (k == label) zl = z;
  }
  s = 0.f;
  for (int k = 0; k < K; ++k) s += expf(px.z(k) - m);
}

// ---- forward.  A thread owns one pixel at a time (consecutive threads = consecutive label bytes of a pixel row) and strides the N S S pixels by
// the grid; per workgroup one loss partial and one valid count go to scratch, and the confusion counts are gathered in an LDS histogram that
// is flushed with one 64-bit integer atomic per non-zero entry.  A second one-workgroup launch folds the partials in a fixed order.
#define SEG_CE_BLOCKS 1024   // at most this many workgroups: scratch holds SEG_CE_BLOCKS floats + SEG_CE_BLOCKS ints
#define SEG_KMAX 64
__global__ __launch_bounds__(256) void seg_ce_kernel(long long npix, int G, int p, int K, const float* __restrict__ pl, const unsigned char* __restrict__ lab,
                                                     float* __restrict__ part, int* __restrict__ cpart, unsigned long long* __restrict__ conf,
                                                     unsigned char* __restrict__ pred) {
  __shared__ int hist[SEG_KMAX * SEG_KMAX];
  __shared__ float red[17];
  const int S = G * p;
  if (conf != nullptr) {
    for (int i = threadIdx.x; i < K * K; i += 256) hist[i] = 0;
    __syncthreads();
  }
  float loss = 0.f;
  int valid = 0;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < npix; idx += (long long)gridDim.x * 256) {
    const int label = lab != nullptr ? (int)lab[idx] : CSMAE_SEG_IGNORE;
    if (label == CSMAE_SEG_IGNORE && pred == nullptr) continue;
    const int x = (int)(idx % S), y = (int)((idx / S) % S);
    const long long n = idx / ((long long)S * S);
    const SegPixel px = seg_pixel(pl + n * G * G * K, G, K, seg_axis(y, p, G), seg_axis(x, p, G));
    float m, s, zl;
    int arg;
    seg_softmax_stats(px, K, label, m, arg, s, zl);
    if (pred != nullptr) pred[idx] = (unsigned char)arg;
    if (label == CSMAE_SEG_IGNORE) continue;
    loss += (logf(s) + m) - zl;
    valid += 1;
    if (conf != nullptr && label < K) atomicAdd(&hist[label * K + arg], 1);
  }
  loss = block_sum(loss, red);
  const float fv = block_sum((float)valid, red);   // (exact: a workgroup sees fewer than 2^24 pixels — host: N S S < 2^31, over SEG_CE_BLOCKS workgroups once a thread takes a second pixel)
  if (threadIdx.x == 0) { part[blockIdx.x] = loss; cpart[blockIdx.x] = (int)fv; }
  if (conf != nullptr) {   // (block_sum's barriers are behind every LDS atomic)
    for (int i = threadIdx.x; i < K * K; i += 256) {
      const int c = hist[i];
      if (c != 0) atomicAdd(conf + i, (unsigned long long)c);
    }
  }
}
__global__ __launch_bounds__(256) void seg_ce_finish_kernel(int blocks, const float* __restrict__ part, const int* __restrict__ cpart, float* __restrict__ loss,
                                                            long long* __restrict__ count) {
  __shared__ float red[17];
  __shared__ long long cred[256];
  float s = 0.f;
  long long c = 0;
  for (int i = threadIdx.x; i < blocks; i += 256) { s += part[i]; c += cpart[i]; }
  s = block_sum(s, red);
  cred[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 256; ++i) c += cred[i];
    loss[0] = c > 0 ? s / (float)c : 0.f;
    count[0] = c;
  }
}
static int seg_ce_check(const char* what, long long N, int G, int p, int K, int S, const void* pl) {
  CSMAE_REQUIRE(N > 0 && pl, "%s: null or empty argument", what);
  CSMAE_REQUIRE(K >= 2 && K <= SEG_KMAX, "%s: K = %d classes; the kernel holds 2 .. %d", what, K, SEG_KMAX);
  CSMAE_REQUIRE(p == 4 || p == 8 || p == 14 || p == 16, "%s: patch size %d; the kernel takes 4, 8, 14 or 16", what, p);
  CSMAE_REQUIRE(G >= 1 && G <= 4096, "%s: a grid of %d cells per side; the kernel takes 1 .. 4096", what, G);
  CSMAE_REQUIRE(S == G * p, "%s: labels of %d x %d pixels do not fit %d x %d cells of %d pixels", what, S, S, G, G, p);
  CSMAE_REQUIRE(N * S * S <= 0x7fffffffLL, "%s: N S S = %lld pixels are beyond 2^31", what, N * S * S);
  return 0;
}
extern "C" int csmae_seg_ce(long long N, int G, int p, int K, int S, const float* pl, const unsigned char* labels, float* scratch, float* loss, long long* count,
                            long long* conf, unsigned char* pred, void* stream) {
  if (int rc = seg_ce_check("csmae_seg_ce", N, G, p, K, S, pl)) return rc;
  CSMAE_REQUIRE(scratch && loss && count && (labels || pred), "csmae_seg_ce: null argument (scratch: 2048 floats; labels may be absent only with pred)");
  const long long npix = N * S * S;
  const int blocks = (int)min((npix + 255) / 256, (long long)SEG_CE_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(seg_ce_kernel, dim3(blocks), dim3(256), 0, st, npix, G, p, K, pl, labels, scratch, reinterpret_cast<int*>(scratch + SEG_CE_BLOCKS),
                     reinterpret_cast<unsigned long long*>(conf), pred);
  hipLaunchKernelGGL(seg_ce_finish_kernel, dim3(1), dim3(256), 0, st, blocks, scratch, reinterpret_cast<const int*>(scratch + SEG_CE_BLOCKS), loss, count);
  return csmae_check_launch("csmae_seg_ce");
}

// ---- backward, as a gather: one workgroup per cell (n, gy, gx).  The pixels that read the cell lie in rows [p gy - p / 2, p gy + 3 p / 2) and the same
// range of columns, clipped to the image: at most 2 p x 2 p <= 1024.  Pass 1: a thread per footprint pixel recomputes the pixel's log-sum-exp and
// the weight w it gives this cell, into LDS.  Pass 2: lanes across the classes (KP = K rounded up to a power of two; 256 / KP pixel slots side by
// side), each slot walks every (256 / KP)-th pixel and sums w (exp(z_k - lse) - [k == label]); the slots are folded in order.  Every element
// of dpl is written once, from a fixed summation order: nothing to clear, two runs give the same bits.
#define SEG_FOOT 1024
__global__ __launch_bounds__(256) void seg_ce_bwd_kernel(int G, int p, int K, int kp_log2, const float* __restrict__ pl, const unsigned char* __restrict__ lab,
                                                         const long long* __restrict__ count, const float* __restrict__ gscale, float* __restrict__ dpl) {
  __shared__ float s_lse[SEG_FOOT], s_w[SEG_FOOT], s_fy[SEG_FOOT], s_fx[SEG_FOOT];
  __shared__ int s_y0[SEG_FOOT], s_x0[SEG_FOOT];
  __shared__ unsigned char s_lab[SEG_FOOT];
  __shared__ float s_part[256];
  const int S = G * p;
  const long long cell = blockIdx.x;
  const int gx = (int)(cell % G), gy = (int)((cell / G) % G);
  const long long n = cell / ((long long)G * G);
  float* out = dpl + cell * K;
  const long long cnt = count[0];
  if (cnt <= 0) {   // no valid pixel in the batch: the loss is the constant 0
    if (threadIdx.x < K) out[threadIdx.x] = 0.f;
    return;
  }
  const float* pln = pl + n * G * G * K;
  const int ylo = max(p * gy - p / 2, 0), yhi = min(p * gy + 3 * p / 2, S);
  const int xlo = max(p * gx - p / 2, 0), xhi = min(p * gx + 3 * p / 2, S);
  const int fw = xhi - xlo, npx = fw * (yhi - ylo);
  for (int j = threadIdx.x; j < npx; j += 256) {
    const int py = ylo + j / fw, pxx = xlo + j % fw;
    const int label = lab[(n * S + py) * S + pxx];
    float w = 0.f, lse = 0.f;
    const SegAxis ay = seg_axis(py, p, G), ax = seg_axis(pxx, p, G);
    if (label != CSMAE_SEG_IGNORE) {
      const float wy = (ay.i0 == gy ? 1.f - ay.f : 0.f) + (ay.i1 == gy ? ay.f : 0.f);
      const float wx = (ax.i0 == gx ? 1.f - ax.f : 0.f) + (ax.i1 == gx ? ax.f : 0.f);
      w = wy * wx;
      if (w != 0.f) {
        float m, s, zl;
        int arg;
        seg_softmax_stats(seg_pixel(pln, G, K, ay, ax), K, label, m, arg, s, zl);
        lse = logf(s) + m;
      }
    }
    s_w[j] = w; s_lse[j] = lse; s_lab[j] = (unsigned char)label;
    s_fy[j] = ay.f; s_fx[j] = ax.f; s_y0[j] = ay.i0; s_x0[j] = ax.i0;
  }
  __syncthreads();
  const int k = threadIdx.x & ((1 << kp_log2) - 1), slot = threadIdx.x >> kp_log2, nslots = 256 >> kp_log2;
  float acc = 0.f;
  if (k < K) {
    for (int j = slot; j < npx; j += nslots) {
      const float w = s_w[j];
      if (w == 0.f) continue;
      SegAxis ay, ax;
      ay.i0 = s_y0[j]; ay.i1 = min(ay.i0 + 1, G - 1); ay.f = s_fy[j];
      ax.i0 = s_x0[j]; ax.i1 = min(ax.i0 + 1, G - 1); ax.f = s_fx[j];
      const float z = seg_pixel(pln, G, K, ay, ax).z(k);
      acc += w * (expf(z - s_lse[j]) - (k == (int)s_lab[j] ? 1.f : 0.f));
    }
  }
  s_part[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < K) {
    float t = s_part[threadIdx.x];
    for (int sl = 1; sl < nslots; ++sl) t += s_part[(sl << kp_log2) + threadIdx.x];
    const float g = gscale != nullptr ? gscale[0] : 1.f;
    out[threadIdx.x] = t * (g / (float)cnt);
  }
}
extern "C" int csmae_seg_ce_bwd(long long N, int G, int p, int K, int S, const float* pl, const unsigned char* labels, const long long* count, const float* gscale,
                                float* dpl, void* stream) {
  if (int rc = seg_ce_check("csmae_seg_ce_bwd", N, G, p, K, S, pl)) return rc;
  CSMAE_REQUIRE(labels && count && dpl, "csmae_seg_ce_bwd: null argument (count: the device scalar csmae_seg_ce wrote)");
  CSMAE_REQUIRE(N * G * G <= 0x7fffffffLL, "csmae_seg_ce_bwd: N G G = %lld cells are beyond the grid", N * G * G);
  int kp_log2 = 1;
  while ((1 << kp_log2) < K) ++kp_log2;
  hipLaunchKernelGGL(seg_ce_bwd_kernel, dim3((unsigned)(N * G * G)), dim3(256), 0, (hipStream_t)stream, G, p, K, kp_log2, pl, labels, count, gscale, dpl);
  return csmae_check_launch("csmae_seg_ce_bwd");
}
