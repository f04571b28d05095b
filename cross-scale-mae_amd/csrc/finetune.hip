// End-to-end fine-tuning of the encoder (main_finetune.py, engine_finetune.py): what linear probing (linprobe.hip) lacks.  No arithmetic to speak
// of, so by op / byte count all of it is memory- or latency-bound (no kernel here has been profiled on its own; together with the classifier
// and the loss they are what a 17.8 ms ViT-B step spends behind the last block); 16-byte accesses where the geometry allows, scalar variants
// elsewhere; no atomics, fixed summation orders.
//   probe_pool_bwd   dfeat [N, D] -> the whole residual-stream gradient [N, T, D] through LayerNorm and the pooling, dgamma / dbeta
//   head_linear_dx   dfeat = gscale dlogits W
//   soft_ce          soft-target cross-entropy (timm SoftTargetCrossEntropy) with its gradient
//   mixup_target     dense targets from labels: label smoothing + the mix with the flipped batch (timm mixup_target)
//   mixup_cutmix     batch-mode mixup / cutmix of the images with the flipped batch, out of place
//   pos_embed_grad   dpos[t] (+)= sum_n dres[n, t]
#include "common.h"
#include "probe_common.h"

// V consecutive floats -> V elements of T (pointer V-element aligned)
template <typename T, int V> __device__ __forceinline__ void ft_st(T* p, const float* v);
template <> __device__ __forceinline__ void ft_st<float, 1>(float* p, const float* v) { p[0] = v[0]; }
template <> __device__ __forceinline__ void ft_st<float, 4>(float* p, const float* v) { *reinterpret_cast<f4_t*>(p) = f4_t{v[0], v[1], v[2], v[3]}; }
template <> __device__ __forceinline__ void ft_st<bf16_t, 4>(bf16_t* p, const float* v) { st4<bf16_t>(p, f4_t{v[0], v[1], v[2], v[3]}); }
template <> __device__ __forceinline__ void ft_st<bf16_t, 8>(bf16_t* p, const float* v) {
  *reinterpret_cast<uint4*>(p) = make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
}
template <typename T, int V> __device__ __forceinline__ void ft_ld(const T* p, float* v) { pool_ld<T, V>(p, v); }
template <> __device__ __forceinline__ void ft_ld<float, 1>(const float* p, float* v) { v[0] = p[0]; }
template <> __device__ __forceinline__ void ft_ld<bf16_t, 1>(const bf16_t* p, float* v) { v[0] = bf2f(p[0]); }

// ---- pooling + final norm, backward.  One workgroup per sample, as the forward (at batch 128 that is 128 workgroups: half the CUs write the
// sample's T rows; splitting the write over more workgroups would need the pooled row recomputed or staged per workgroup — not done, unmeasured): it recomputes the pooled row and its statistics, applies the
// LayerNorm backward (dp = rstd (g - mean(g) - xhat mean(g xhat)), g = dfeat gamma), leaves dfeat xhat / dfeat as the sample's partial row of
// dgamma / dbeta, and writes all T rows of the sample's gradient: dp / (t1 - t0) into rows [t0, t1), zero elsewhere.
template <typename T, int V>
__global__ __launch_bounds__(POOL_THREADS) void probe_pool_bwd_kernel(int T_, int D, int t0, int t1, const T* __restrict__ x, const float* __restrict__ dfeat,
                                                                      const float* __restrict__ gamma, float eps, T* __restrict__ dres, float* __restrict__ part) {
  __shared__ float acc[POOL_LDS];
  __shared__ float red[17];
  float mean, rstd;
  pool_row_stats<T, V>(D, t0, t1, x + (long long)blockIdx.x * T_ * D, eps, acc, red, mean, rstd);
  const float* df = dfeat + (long long)blockIdx.x * D;
  float* pr = part + (long long)blockIdx.x * 2 * D;
  float s1 = 0.f, s2 = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    const float xh = (acc[d] - mean) * rstd, dv = df[d], g = dv * gamma[d];
    s1 += g;
    s2 = fmaf(g, xh, s2);
    pr[d] = dv * xh;
    pr[D + d] = dv;
  }
  s1 = block_sum(s1, red) / (float)D;
  s2 = block_sum(s2, red) / (float)D;
  const float scale = rstd / (float)(t1 - t0);
  for (int d = threadIdx.x; d < D; d += blockDim.x) {   // (thread d is the only reader of acc[d] so far)
    const float xh = (acc[d] - mean) * rstd, g = df[d] * gamma[d];
    acc[d] = scale * ((g - s1) - xh * s2);
  }
  __syncthreads();
  const int groups = D / V, lanes = POOL_THREADS / groups;
  const int cg = threadIdx.x % groups, tl = threadIdx.x / groups;
  if (tl >= lanes) return;
  T* out = dres + (long long)blockIdx.x * T_ * D + cg * V;
  for (int t = tl; t < T_; t += lanes) {
    const bool live = t >= t0 && t < t1;
    float v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = live ? acc[cg * V + k] : 0.f;
    ft_st<T, V>(out + (long long)t * D, v);
  }
}
// dgamma / dbeta = the samples' partial rows summed in sample order: a thread owns one of the 2 D columns
__global__ __launch_bounds__(256) void probe_pool_fold_kernel(long long N, int D, const float* __restrict__ part, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              int accumulate) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= 2 * D) return;
  float s = 0.f;
  for (long long n = 0; n < N; ++n) s += part[n * 2 * D + c];
  float* dst = c < D ? dgamma + c : dbeta + (c - D);
  *dst = accumulate ? *dst + s : s;
}
extern "C" int csmae_probe_pool_bwd(int dtype, int global_pool, long long N, int T, int D, const void* x, const float* dfeat, const float* gamma, float eps,
                                    void* dres, float* partial, float* dgamma, float* dbeta, int accumulate, void* stream) {
  CSMAE_REQUIRE(N > 0 && N <= 0x7fffffffLL && T >= 1 && D >= 4 && x && dfeat && gamma && dres && partial && dgamma && dbeta,
                "csmae_probe_pool_bwd: null or empty argument (partial: 2 N D floats)");
  CSMAE_REQUIRE(dtype == CSMAE_F32 || dtype == CSMAE_BF16, "csmae_probe_pool_bwd: bad dtype %d", dtype);
  CSMAE_REQUIRE(!(global_pool && T < 2), "csmae_probe_pool_bwd: global_pool averages tokens 1 .. T-1: T = %d leaves nothing to average", T);
  CSMAE_REQUIRE(D % 4 == 0 && D / 4 <= POOL_THREADS, "csmae_probe_pool_bwd: D = %d must be a multiple of 4, at most %d", D, 4 * POOL_THREADS);
  CSMAE_REQUIRE((((uintptr_t)x | (uintptr_t)dres) & 15) == 0, "csmae_probe_pool_bwd: x and dres must be 16-byte aligned");
  const int t0 = global_pool ? 1 : 0, t1 = global_pool ? T : 1;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)N), block(POOL_THREADS);
#define PPB(TT, VV) hipLaunchKernelGGL((probe_pool_bwd_kernel<TT, VV>), grid, block, 0, st, T, D, t0, t1, (const TT*)x, dfeat, gamma, eps, (TT*)dres, partial)
  if (dtype == CSMAE_F32) PPB(float, 4);
  else if (D % 8 == 0) PPB(bf16_t, 8);
  else PPB(bf16_t, 4);
#undef PPB
  hipLaunchKernelGGL(probe_pool_fold_kernel, dim3(cdiv(2 * D, 256)), dim3(256), 0, st, N, D, partial, dgamma, dbeta, accumulate);
  return csmae_check_launch("csmae_probe_pool_bwd");
}

// ---- classifier, gradient of its input.  A thread owns one feature column d (rows of W coalesced over the workgroup), a workgroup HD_ROWS samples
// (dlogits[n, k] is uniform over the workgroup); the classes are walked in order.
#define HD_ROWS 4
__global__ __launch_bounds__(256) void head_linear_dx_kernel(long long N, int D, int K, const float* __restrict__ dl, const float* __restrict__ w,
                                                             const float* __restrict__ gscale, float* __restrict__ dx) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  const long long n0 = (long long)blockIdx.y * HD_ROWS;
  const int rows = (int)min((long long)HD_ROWS, N - n0);
  if (d >= D) return;
  float s[HD_ROWS];
#pragma unroll
  for (int r = 0; r < HD_ROWS; ++r) s[r] = 0.f;
  for (int k = 0; k < K; ++k) {
    const float wv = w[(long long)k * D + d];
#pragma unroll
    for (int r = 0; r < HD_ROWS; ++r)
      if (r < rows) s[r] = fmaf(dl[(n0 + r) * K + k], wv, s[r]);
  }
  const float g = gscale != nullptr ? gscale[0] : 1.f;
#pragma unroll
  for (int r = 0; r < HD_ROWS; ++r)
    if (r < rows) dx[(n0 + r) * D + d] = g * s[r];
}
extern "C" int csmae_head_linear_dx(long long N, int D, int K, const float* dlogits, const float* w, const float* gscale, float* dx, void* stream) {
  CSMAE_REQUIRE(N > 0 && D > 0 && K > 0 && dlogits && w && dx, "csmae_head_linear_dx: null or empty argument");
  CSMAE_REQUIRE(cdiv(N, HD_ROWS) <= 65535, "csmae_head_linear_dx: N = %lld is beyond the grid (at most %d rows)", N, 65535 * HD_ROWS);
  hipLaunchKernelGGL(head_linear_dx_kernel, dim3(cdiv(D, 256), cdiv(N, HD_ROWS)), dim3(256), 0, (hipStream_t)stream, N, D, K, dlogits, w, gscale, dx);
  return csmae_check_launch("csmae_head_linear_dx");
}

// ---- soft-target cross-entropy: loss = mean_n sum_k -t[n, k] log_softmax(z)[n, k], dlogits = gout (softmax sum_k t - t) / N.  One workgroup per row,
// stable form; the row's loss is summed as t ((m - z) + log s): non-negative terms, no cancellation against the row maximum m.  Row losses go to
// scratch [N], a one-workgroup launch folds them in a fixed order (the layout of csmae_softmax_ce).  V = 4: rows of K % 4 == 0 floats, 16-byte accesses.
__device__ __forceinline__ float ft_block_max(float v, float* smem /* >= 17 floats */) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) smem[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) { float s = smem[0]; for (int i = 1; i < nw; ++i) s = fmaxf(s, smem[i]); smem[16] = s; }
  __syncthreads();
  return smem[16];
}
template <int V>
__global__ __launch_bounds__(256) void soft_ce_rows_kernel(long long N, int K, const float* __restrict__ logits, const float* __restrict__ target,
                                                           const float* __restrict__ gout, float* __restrict__ scratch, float* __restrict__ dlogits) {
  __shared__ float red[17];
  const long long n = blockIdx.x;
  const float* row = logits + n * K;
  const float* trow = target + n * K;
  float m = -INFINITY;
  for (int k = threadIdx.x * V; k < K; k += blockDim.x * V) {
    float z[V];
    ft_ld<float, V>(row + k, z);
#pragma unroll
    for (int j = 0; j < V; ++j) m = fmaxf(m, z[j]);
  }
  m = ft_block_max(m, red);
  float s = 0.f, ts = 0.f, a = 0.f;
  for (int k = threadIdx.x * V; k < K; k += blockDim.x * V) {
    float z[V], t[V];
    ft_ld<float, V>(row + k, z);
    ft_ld<float, V>(trow + k, t);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      s += expf(z[j] - m);
      ts += t[j];
      a = fmaf(t[j], m - z[j], a);
    }
  }
  s = block_sum(s, red);
  ts = block_sum(ts, red);
  a = block_sum(a, red);
  if (threadIdx.x == 0) scratch[n] = fmaf(logf(s), ts, a);
  if (dlogits != nullptr) {
    const float g = (gout != nullptr ? gout[0] : 1.f) / (float)N, inv = ts / s;
    float* drow = dlogits + n * K;
    for (int k = threadIdx.x * V; k < K; k += blockDim.x * V) {
      float z[V], t[V], o[V];
      ft_ld<float, V>(row + k, z);
      ft_ld<float, V>(trow + k, t);
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = g * (expf(z[j] - m) * inv - t[j]);
      ft_st<float, V>(drow + k, o);
    }
  }
}
__global__ __launch_bounds__(256) void soft_ce_finish_kernel(long long N, const float* __restrict__ scratch, float* __restrict__ loss) {
  __shared__ float red[17];
  float a = 0.f;
  for (long long n = threadIdx.x; n < N; n += blockDim.x) a += scratch[n];
  a = block_sum(a, red);
  if (threadIdx.x == 0) loss[0] = a / (float)N;
}
static inline bool ft_vec4(int K, const void* a, const void* b, const void* c) {
  return K % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}
extern "C" int csmae_soft_ce(long long N, int K, const float* logits, const float* target, const float* gout, float* scratch, float* loss, float* dlogits,
                             void* stream) {
  CSMAE_REQUIRE(N > 0 && N <= 0x7fffffffLL && K > 0 && logits && target && scratch && loss, "csmae_soft_ce: null or empty argument (scratch: N floats)");
  hipStream_t st = (hipStream_t)stream;
  if (ft_vec4(K, logits, target, dlogits)) hipLaunchKernelGGL(soft_ce_rows_kernel<4>, dim3((unsigned)N), dim3(256), 0, st, N, K, logits, target, gout, scratch, dlogits);
  else hipLaunchKernelGGL(soft_ce_rows_kernel<1>, dim3((unsigned)N), dim3(256), 0, st, N, K, logits, target, gout, scratch, dlogits);
  hipLaunchKernelGGL(soft_ce_finish_kernel, dim3(1), dim3(256), 0, st, N, scratch, loss);
  return csmae_check_launch("csmae_soft_ce");
}

// ---- dense targets (timm mixup_target): t[n] = lam onehot(y[n], on, off) + (1 - lam) onehot(y[N - 1 - n], on, off), off = smoothing / K,
// on = 1 - smoothing + off.  A label is only ever compared with the class index: one outside [0, K) indexes nothing (its row is `off` throughout).
template <int V>
__global__ __launch_bounds__(256) void mixup_target_kernel(long long N, int K, const long long* __restrict__ labels, float lam, float on, float off,
                                                           float* __restrict__ target) {
  const long long n = blockIdx.y;
  const int k0 = (blockIdx.x * 256 + threadIdx.x) * V;
  if (k0 >= K) return;
  const long long ya = labels[n], yb = labels[N - 1 - n];
  const float oml = 1.f - lam;
  float o[V];
#pragma unroll
  for (int j = 0; j < V; ++j) o[j] = lam * ((k0 + j) == ya ? on : off) + oml * ((k0 + j) == yb ? on : off);
  ft_st<float, V>(target + n * K + k0, o);
}
extern "C" int csmae_mixup_target(long long N, int K, const long long* labels, float lam, float smoothing, float* target, void* stream) {
  CSMAE_REQUIRE(N > 0 && N <= 65535 && K > 0 && labels && target, "csmae_mixup_target: null or empty argument (N <= 65535)");
  CSMAE_REQUIRE(lam >= 0.f && lam <= 1.f && smoothing >= 0.f && smoothing < 1.f, "csmae_mixup_target: lam = %g must lie in [0, 1], smoothing = %g in [0, 1)",
                (double)lam, (double)smoothing);
  const float off = smoothing / (float)K, on = 1.f - smoothing + off;
  hipStream_t st = (hipStream_t)stream;
  if (ft_vec4(K, target, nullptr, nullptr)) hipLaunchKernelGGL(mixup_target_kernel<4>, dim3(cdiv(K, 1024), (unsigned)N), dim3(256), 0, st, N, K, labels, lam, on, off, target);
  else hipLaunchKernelGGL(mixup_target_kernel<1>, dim3(cdiv(K, 256), (unsigned)N), dim3(256), 0, st, N, K, labels, lam, on, off, target);
  return csmae_check_launch("csmae_mixup_target");
}

// ---- batch-mode mixup / cutmix (timm Mixup._mix_batch): sample n is mixed with sample N - 1 - n, which is why the result goes to a second buffer.
//   mixup:  out[n] = lam x[n] + (1 - lam) x[N - 1 - n]   (two rounded products and one rounded sum, as torch's mul / add)
//   cutmix: out[n] = x[n], but x[N - 1 - n] inside rows [yl, yh) x columns [xl, xh)
// A sample is walked as one flat run of C H W floats (V = 4 when that is a multiple of 4: a vector may straddle image rows, the box test is per
// element); blockIdx.y = the sample.
template <int V>
__global__ __launch_bounds__(256) void mixup_cutmix_kernel(int N, int chw, int H, int W, const float* __restrict__ x, float* __restrict__ out, int cutmix, float lam,
                                                           int yl, int yh, int xl, int xh) {
  const int n = blockIdx.y;
  const int i0 = (blockIdx.x * 256 + threadIdx.x) * V;
  if (i0 >= chw) return;
  const float* a = x + (long long)n * chw + i0;
  const float* b = x + (long long)(N - 1 - n) * chw + i0;
  float va[V], vb[V], o[V];
  ft_ld<float, V>(a, va);
  ft_ld<float, V>(b, vb);
  if (cutmix) {
    int col = i0 % W, rowi = (i0 / W) % H;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      o[j] = (rowi >= yl && rowi < yh && col >= xl && col < xh) ? vb[j] : va[j];
      if (++col == W) { col = 0; if (++rowi == H) rowi = 0; }
    }
  } else {
#pragma clang fp contract(off)   // (no fused multiply-add: the two products are rounded before the sum)
    const float oml = 1.f - lam;
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = lam * va[j] + oml * vb[j];
  }
  ft_st<float, V>(out + (long long)n * chw + i0, o);
}
extern "C" int csmae_mixup_cutmix(int cutmix, long long N, int C, int H, int W, const float* x, float* out, float lam, int yl, int yh, int xl, int xh, void* stream) {
  CSMAE_REQUIRE(N > 0 && N <= 65535 && C > 0 && H > 0 && W > 0 && x && out && x != out, "csmae_mixup_cutmix: null, empty or aliased argument (out of place, N <= 65535)");
  CSMAE_REQUIRE(N % 2 == 0, "csmae_mixup_cutmix: batch size %lld should be even (sample n is mixed with sample N - 1 - n)", N);
  CSMAE_REQUIRE((long long)C * H * W <= 0x7fffffffLL, "csmae_mixup_cutmix: C H W = %lld is beyond 2^31", (long long)C * H * W);
  if (cutmix) CSMAE_REQUIRE(0 <= yl && yl <= yh && yh <= H && 0 <= xl && xl <= xh && xh <= W, "csmae_mixup_cutmix: box [%d, %d) x [%d, %d) outside the %d x %d image", yl, yh, xl, xh, H, W);
  else CSMAE_REQUIRE(lam >= 0.f && lam <= 1.f, "csmae_mixup_cutmix: lam = %g must lie in [0, 1]", (double)lam);
  const int chw = C * H * W;
  hipStream_t st = (hipStream_t)stream;
  if (ft_vec4(chw, x, out, nullptr)) hipLaunchKernelGGL(mixup_cutmix_kernel<4>, dim3(cdiv(chw, 1024), (unsigned)N), dim3(256), 0, st, (int)N, chw, H, W, x, out, cutmix, lam, yl, yh, xl, xh);
  else hipLaunchKernelGGL(mixup_cutmix_kernel<1>, dim3(cdiv(chw, 256), (unsigned)N), dim3(256), 0, st, (int)N, chw, H, W, x, out, cutmix, lam, yl, yh, xl, xh);
  return csmae_check_launch("csmae_mixup_cutmix");
}

// ---- position-embedding gradient: dpos [T, D] (+)= sum_n dres[n] over the flat run of T D elements; a thread owns V consecutive elements and walks
// the samples in order, fp32 accumulation.  (Valid because fine-tuning keeps the token order: row t of every sample took pos_embed[t].)
template <typename T, int V>
__global__ __launch_bounds__(256) void pos_embed_grad_kernel(long long N, long long td, const T* __restrict__ dres, float* __restrict__ dpos, int accumulate) {
  const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
  if (i0 >= td) return;
  float s[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s[j] = 0.f;
  for (long long n = 0; n < N; ++n) {
    float v[V];
    ft_ld<T, V>(dres + n * td + i0, v);
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] += v[j];
  }
  constexpr int W = V >= 4 ? 4 : 1;   // 16-byte reads / writes of the fp32 result (dpos is 16-byte aligned whenever V > 1)
#pragma unroll
  for (int j = 0; j < V; j += W) {
    if (accumulate) {
      float o[W];
      ft_ld<float, W>(dpos + i0 + j, o);
#pragma unroll
      for (int k = 0; k < W; ++k) s[j + k] += o[k];
    }
    ft_st<float, W>(dpos + i0 + j, s + j);
  }
}
extern "C" int csmae_pos_embed_grad(int dtype, long long N, int T, int D, const void* dres, float* dpos, int accumulate, void* stream) {
  CSMAE_REQUIRE(N > 0 && T > 0 && D > 0 && dres && dpos, "csmae_pos_embed_grad: null or empty argument");
  CSMAE_REQUIRE(dtype == CSMAE_F32 || dtype == CSMAE_BF16, "csmae_pos_embed_grad: bad dtype %d", dtype);
  const long long td = (long long)T * D;
  const bool al = (((uintptr_t)dres | (uintptr_t)dpos) & 15) == 0;
  CSMAE_REQUIRE(cdiv(td, 256) <= 0x7fffffff, "csmae_pos_embed_grad: T D = %lld is beyond the grid", td);
  hipStream_t st = (hipStream_t)stream;
#define PEG(TT, VV) hipLaunchKernelGGL((pos_embed_grad_kernel<TT, VV>), dim3(cdiv(td, 256 * VV)), dim3(256), 0, st, N, td, (const TT*)dres, dpos, accumulate)
  if (dtype == CSMAE_F32) { if (al && td % 4 == 0) PEG(float, 4); else PEG(float, 1); }
  else if (al && td % 8 == 0) PEG(bf16_t, 8);
  else if (al && td % 4 == 0) PEG(bf16_t, 4);
  else PEG(bf16_t, 1);
#undef PEG
  return csmae_check_launch("csmae_pos_embed_grad");
}
