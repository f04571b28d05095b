// Downstream classification (main_linprobe.py, main_finetune.py, engine_finetune.py): every kernel that only linear probing and end-to-end
// fine-tuning use, in the order the data flows through a step.  All arithmetic is fp32; only the token stream (and its gradient) may be bf16.
// The kernels are small and HBM- / latency-bound (N x D x K is three orders of magnitude below one trunk forward; together they are what a
// 17.8 ms ViT-B fine-tune step spends behind the last block; none has been profiled on its own): plain fp32 with fp32 accumulation, no MFMA
// route, 16-byte accesses where the geometry allows and scalar variants elsewhere, no atomics, fixed summation orders.
//   mixup_cutmix     batch-mode mixup / cutmix of the images with the flipped batch, out of place
//   mixup_target     dense targets from labels: label smoothing + the mix with the flipped batch (timm mixup_target)
//   probe_pool_fwd   mean over the patch tokens (or the cls token) + LayerNorm -> feat [N, D]
//   bn1d_fwd         BatchNorm1d(D, affine=False) over the batch axis of feat, running statistics in training mode
//   head_linear_fwd  logits = fbn W^T + b
//   softmax_ce       mean cross-entropy, dlogits, top-1 / top-5 counts
//   soft_ce          soft-target cross-entropy (timm SoftTargetCrossEntropy) with its gradient
//   head_linear_bwd  dW = gscale dlogits^T fbn, db = gscale sum_n dlogits
//   head_linear_dx   dfeat = gscale dlogits W
//   probe_pool_bwd   dfeat [N, D] -> the whole residual-stream gradient [N, T, D] through LayerNorm and the pooling, dgamma / dbeta
//   pos_embed_grad   dpos[t] (+)= sum_n dres[n, t]
//   lars_step        LARS over a pointer table of tensors: partial squared norms, then the update
#include "common.h"

// V consecutive elements of T <-> V floats, (T, V) in {float, bf16_t} x {1, 4, 8} (pointer V-element aligned; 8 bf16 = one 16-byte access)
template <typename T, int V> __device__ __forceinline__ void ldv(const T* p, float* v) {
  if constexpr (V == 1) {
    v[0] = ld_as_f32<T>(p);
  } else if constexpr (V == 4) {
    const f4_t a = ld4<T>(p);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
  } else {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
    v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
    v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u);
    v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
  }
}
template <typename T, int V> __device__ __forceinline__ void stv(T* p, const float* v) {
  if constexpr (V == 1) st_from_f32<T>(p, v[0]);
  else if constexpr (V == 4) st4<T>(p, f4_t{v[0], v[1], v[2], v[3]});
  else *reinterpret_cast<uint4*>(p) = make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
}
// the 16-byte variant of a kernel over rows of n floats: n a multiple of 4 and every given pointer 16-byte aligned
static inline bool vec4_ok(long long n, const void* a, const void* b = nullptr, const void* c = nullptr) {
  return n % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}
__device__ __forceinline__ float block_max(float v, float* smem /* >= 17 floats */) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) smem[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) { float s = smem[0]; for (int i = 1; i < nw; ++i) s = fmaxf(s, smem[i]); smem[16] = s; }
  __syncthreads();
  return smem[16];
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
  ldv<float, V>(a, va);
  ldv<float, V>(b, vb);
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
  stv<float, V>(out + (long long)n * chw + i0, o);
}
extern "C" int csmae_mixup_cutmix(int cutmix, long long N, int C, int H, int W, const float* x, float* out, float lam, int yl, int yh, int xl, int xh, void* stream) {
  CSMAE_REQUIRE(N > 0 && N <= 65535 && C > 0 && H > 0 && W > 0 && x && out && x != out, "csmae_mixup_cutmix: null, empty or aliased argument (out of place, N <= 65535)");
  CSMAE_REQUIRE(N % 2 == 0, "csmae_mixup_cutmix: batch size %lld should be even (sample n is mixed with sample N - 1 - n)", N);
  CSMAE_REQUIRE((long long)C * H * W <= 0x7fffffffLL, "csmae_mixup_cutmix: C H W = %lld is beyond 2^31", (long long)C * H * W);
  if (cutmix) CSMAE_REQUIRE(0 <= yl && yl <= yh && yh <= H && 0 <= xl && xl <= xh && xh <= W, "csmae_mixup_cutmix: box [%d, %d) x [%d, %d) outside the %d x %d image", yl, yh, xl, xh, H, W);
  else CSMAE_REQUIRE(lam >= 0.f && lam <= 1.f, "csmae_mixup_cutmix: lam = %g must lie in [0, 1]", (double)lam);
  const int chw = C * H * W;
  hipStream_t st = (hipStream_t)stream;
  if (vec4_ok(chw, x, out)) hipLaunchKernelGGL(mixup_cutmix_kernel<4>, dim3(cdiv(chw, 1024), (unsigned)N), dim3(256), 0, st, (int)N, chw, H, W, x, out, cutmix, lam, yl, yh, xl, xh);
  else hipLaunchKernelGGL(mixup_cutmix_kernel<1>, dim3(cdiv(chw, 256), (unsigned)N), dim3(256), 0, st, (int)N, chw, H, W, x, out, cutmix, lam, yl, yh, xl, xh);
  return csmae_check_launch("csmae_mixup_cutmix");
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
  stv<float, V>(target + n * K + k0, o);
}
extern "C" int csmae_mixup_target(long long N, int K, const long long* labels, float lam, float smoothing, float* target, void* stream) {
  CSMAE_REQUIRE(N > 0 && N <= 65535 && K > 0 && labels && target, "csmae_mixup_target: null or empty argument (N <= 65535)");
  CSMAE_REQUIRE(lam >= 0.f && lam <= 1.f && smoothing >= 0.f && smoothing < 1.f, "csmae_mixup_target: lam = %g must lie in [0, 1], smoothing = %g in [0, 1)",
                (double)lam, (double)smoothing);
  const float off = smoothing / (float)K, on = 1.f - smoothing + off;
  hipStream_t st = (hipStream_t)stream;
  if (vec4_ok(K, target)) hipLaunchKernelGGL(mixup_target_kernel<4>, dim3(cdiv(K, 1024), (unsigned)N), dim3(256), 0, st, N, K, labels, lam, on, off, target);
  else hipLaunchKernelGGL(mixup_target_kernel<1>, dim3(cdiv(K, 256), (unsigned)N), dim3(256), 0, st, N, K, labels, lam, on, off, target);
  return csmae_check_launch("csmae_mixup_target");
}

// ---- pooling + final norm.  One workgroup per sample; a thread owns V consecutive columns (16 bytes of the row) and every `lanes`-th token, the
// token lanes are folded through LDS, the row statistics through block_sum (two passes: mean, then centred squares).
#define POOL_THREADS 1024
#define POOL_LDS 8192   // floats: lanes * D <= POOL_THREADS * V <= 8192
// the (T, V) instance for a token stream of `dtype` with rows of D elements (host: D % 4 == 0)
#define POOL_DISPATCH(LAUNCH)               \
  do {                                      \
    if (dtype == CSMAE_F32) LAUNCH(float, 4); \
    else if (D % 8 == 0) LAUNCH(bf16_t, 8);   \
    else LAUNCH(bf16_t, 4);                   \
  } while (0)
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
      ldv<T, V>(xs + (long long)t * D + cg * V, v);
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
template <typename T, int V>
__global__ __launch_bounds__(POOL_THREADS) void probe_pool_kernel(int T_, int D, int t0, int t1, const T* __restrict__ x, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float eps, float* __restrict__ feat) {
  __shared__ float acc[POOL_LDS];
  __shared__ float red[17];
  float mean, rstd;
  pool_row_stats<T, V>(D, t0, t1, x + (long long)blockIdx.x * T_ * D, eps, acc, red, mean, rstd);
  float* out = feat + (long long)blockIdx.x * D;
  for (int d = threadIdx.x; d < D; d += blockDim.x) out[d] = (acc[d] - mean) * rstd * gamma[d] + beta[d];
}
extern "C" int csmae_probe_pool_fwd(int dtype, int global_pool, long long N, int T, int D, const void* x, const float* gamma, const float* beta, float eps,
                                    float* feat, void* stream) {
  CSMAE_REQUIRE(N > 0 && N <= 0x7fffffffLL && T >= 1 && D >= 4 && x && gamma && beta && feat, "csmae_probe_pool_fwd: null or empty argument");
  CSMAE_REQUIRE(dtype == CSMAE_F32 || dtype == CSMAE_BF16, "csmae_probe_pool_fwd: bad dtype %d", dtype);
  CSMAE_REQUIRE(!(global_pool && T < 2), "csmae_probe_pool_fwd: global_pool averages tokens 1 .. T-1: T = %d leaves nothing to average", T);
  CSMAE_REQUIRE(D % 4 == 0 && D / 4 <= POOL_THREADS, "csmae_probe_pool_fwd: D = %d must be a multiple of 4, at most %d", D, 4 * POOL_THREADS);
  CSMAE_REQUIRE(((uintptr_t)x & 15) == 0, "csmae_probe_pool_fwd: x must be 16-byte aligned");
  const int t0 = global_pool ? 1 : 0, t1 = global_pool ? T : 1;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)N), block(POOL_THREADS);
#define PPF(TT, VV) hipLaunchKernelGGL((probe_pool_kernel<TT, VV>), grid, block, 0, st, T, D, t0, t1, (const TT*)x, gamma, beta, eps, feat)
  POOL_DISPATCH(PPF);
#undef PPF
  return csmae_check_launch("csmae_probe_pool_fwd");
}

// Backward.  One workgroup per sample, as the forward (at batch 128 that is 128 workgroups: half the CUs write the sample's T rows; splitting
// the write over more workgroups would need the pooled row recomputed or staged per workgroup — not done, unmeasured): it recomputes the
// pooled row and its statistics, applies the LayerNorm backward (dp = rstd (g - mean(g) - xhat mean(g xhat)), g = dfeat gamma), leaves
// dfeat xhat / dfeat as the sample's partial row of dgamma / dbeta, and writes all T rows of the sample's gradient: dp / (t1 - t0) into rows
// [t0, t1), zero elsewhere.
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
    stv<T, V>(out + (long long)t * D, v);
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
  POOL_DISPATCH(PPB);
#undef PPB
  hipLaunchKernelGGL(probe_pool_fold_kernel, dim3(cdiv(2 * D, 256)), dim3(256), 0, st, N, D, partial, dgamma, dbeta, accumulate);
  return csmae_check_launch("csmae_probe_pool_bwd");
}

// ---- BatchNorm1d(D, affine=False) over the batch axis.  A workgroup owns 64 columns (tx) with 4 row lanes (ty); three passes over its
// [N, 64] slab (the second and third come from cache): mean, centred squares, normalise.
__device__ __forceinline__ float bn_fold(float v, float (*red)[64], int tx, int ty) {
  __syncthreads();
  red[ty][tx] = v;
  __syncthreads();
  return (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
}
__global__ __launch_bounds__(256) void bn1d_kernel(long long N, int D, const float* __restrict__ x, float eps, float momentum, float* __restrict__ y,
                                                   float* __restrict__ running_mean, float* __restrict__ running_var, long long* __restrict__ nbt, int training) {
  __shared__ float red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + tx;
  const bool live = col < D;
  float mean, var;
  if (training) {
    float s = 0.f;
    if (live) for (long long r = ty; r < N; r += 4) s += x[r * D + col];
    mean = bn_fold(s, red, tx, ty) / (float)N;
    s = 0.f;
    if (live) for (long long r = ty; r < N; r += 4) { const float c = x[r * D + col] - mean; s += c * c; }
    const float ss = bn_fold(s, red, tx, ty);
    var = ss / (float)N;                      // biased: what normalises
    if (live && ty == 0) {                    // running statistics take the unbiased variance (torch.nn.BatchNorm1d)
      running_mean[col] = (1.f - momentum) * running_mean[col] + momentum * mean;
      running_var[col] = (1.f - momentum) * running_var[col] + momentum * (ss / (float)(N - 1));
    }
    if (nbt != nullptr && blockIdx.x == 0 && threadIdx.x == 0) nbt[0] += 1;
  } else {
    mean = live ? running_mean[col] : 0.f;
    var = live ? running_var[col] : 1.f;
  }
  const float rstd = rsqrtf(var + eps);
  if (live) for (long long r = ty; r < N; r += 4) y[r * D + col] = (x[r * D + col] - mean) * rstd;
}
extern "C" int csmae_bn1d_fwd(long long N, int D, const float* feat, float eps, float momentum, float* fbn, float* running_mean, float* running_var,
                              long long* num_batches_tracked, int training, void* stream) {
  CSMAE_REQUIRE(N > 0 && D > 0 && feat && fbn && running_mean && running_var, "csmae_bn1d_fwd: null or empty argument");
  CSMAE_REQUIRE(!(training && N < 2), "csmae_bn1d_fwd: training mode needs more than one sample per feature (N = %lld)", N);
  hipLaunchKernelGGL(bn1d_kernel, dim3(cdiv(D, 64)), dim3(256), 0, (hipStream_t)stream, N, D, feat, eps, momentum, fbn, running_mean, running_var,
                     num_batches_tracked, training);
  return csmae_check_launch("csmae_bn1d_fwd");
}

// ---- classifier.  Forward: a wave owns HL_ROWS rows of x and HL_KPW consecutive classes; lanes stride the feature axis (coalesced rows of W and x),
// one wave_sum per output.  Any K, any D.
#define HL_ROWS 4
#define HL_KPW 8
__global__ __launch_bounds__(256) void head_linear_fwd_kernel(long long N, int D, int K, const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ b, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long n0 = (long long)blockIdx.y * HL_ROWS;
  const int k0 = (blockIdx.x * 4 + wave) * HL_KPW;
  if (k0 >= K) return;
  const int rows = (int)min((long long)HL_ROWS, N - n0);
  for (int k = k0; k < min(k0 + HL_KPW, K); ++k) {
    const float* wr = w + (long long)k * D;
    float s[HL_ROWS];
#pragma unroll
    for (int r = 0; r < HL_ROWS; ++r) s[r] = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float wv = wr[d];
#pragma unroll
      for (int r = 0; r < HL_ROWS; ++r)
        if (r < rows) s[r] = fmaf(x[(n0 + r) * D + d], wv, s[r]);
    }
    const float bias = b != nullptr ? b[k] : 0.f;
#pragma unroll
    for (int r = 0; r < HL_ROWS; ++r) {
      const float t = wave_sum(s[r]);
      if (lane == 0 && r < rows) out[(n0 + r) * K + k] = t + bias;
    }
  }
}
extern "C" int csmae_head_linear_fwd(long long N, int D, int K, const float* x, const float* w, const float* b, float* logits, void* stream) {
  CSMAE_REQUIRE(N > 0 && D > 0 && K > 0 && x && w && logits, "csmae_head_linear_fwd: null or empty argument");
  CSMAE_REQUIRE(cdiv(N, HL_ROWS) <= 65535, "csmae_head_linear_fwd: N = %lld is beyond the grid (at most %d rows)", N, 65535 * HL_ROWS);
  hipLaunchKernelGGL(head_linear_fwd_kernel, dim3(cdiv(K, 4 * HL_KPW), cdiv(N, HL_ROWS)), dim3(256), 0, (hipStream_t)stream, N, D, K, x, w, b, logits);
  return csmae_check_launch("csmae_head_linear_fwd");
}

// ---- the two criteria.  One workgroup per row, stable form (row maximum subtracted); row results go to scratch [cols][N], a one-workgroup launch
// folds them column by column in a fixed order: loss[0] = the mean of column 0; with the three columns of csmae_softmax_ce, columns 1 and 2
// are the top-1 / top-5 hits that go to counts.
__global__ __launch_bounds__(256) void ce_finish_kernel(long long N, int cols, const float* __restrict__ scratch, float* __restrict__ loss, float* __restrict__ counts,
                                                        int accumulate_counts) {
  __shared__ float red[17];
  float s[3] = {0.f, 0.f, 0.f};
  for (int j = 0; j < cols; ++j) {
    float a = 0.f;
    for (long long n = threadIdx.x; n < N; n += blockDim.x) a += scratch[j * N + n];
    s[j] = block_sum(a, red);
  }
  if (threadIdx.x == 0) {
    loss[0] = s[0] / (float)N;
    if (cols == 3 && counts != nullptr) {
      counts[0] = accumulate_counts ? counts[0] + s[1] : s[1];
      counts[1] = accumulate_counts ? counts[1] + s[2] : s[2];
    }
  }
}
// Softmax cross-entropy (torch.nn.CrossEntropyLoss, mean) with its gradient and the top-1 / top-5 hit counts (timm `accuracy`); scratch [3][N] =
// {loss, top-1 hit, top-5 hit}.  A row counts toward top-k when fewer than min(k, K) logits are strictly greater than the label's.  A label
// outside [0, K) indexes nothing: its row's loss and gradient are NaN and it scores no hit.
__global__ __launch_bounds__(256) void softmax_ce_rows_kernel(long long N, int K, const float* __restrict__ logits, const long long* __restrict__ labels,
                                                              const float* __restrict__ gout, float* __restrict__ scratch, float* __restrict__ dlogits) {
  __shared__ float red[17];
  const long long n = blockIdx.x;
  const float* row = logits + n * K;
  const long long lab = labels[n];
  const bool ok = lab >= 0 && lab < K;
  float m = -INFINITY;
  for (int k = threadIdx.x; k < K; k += blockDim.x) m = fmaxf(m, row[k]);
  m = block_max(m, red);
  const float ll = ok ? row[lab] : NAN;
  float s = 0.f, above = 0.f;
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    const float v = row[k];
    s += expf(v - m);
    above += (ok && v > ll) ? 1.f : 0.f;
  }
  s = block_sum(s, red);
  above = block_sum(above, red);
  if (threadIdx.x == 0) {
    scratch[n] = ok ? (logf(s) + m) - ll : NAN;
    scratch[N + n] = (ok && above < (float)min(1, K)) ? 1.f : 0.f;
    scratch[2 * N + n] = (ok && above < (float)min(5, K)) ? 1.f : 0.f;
  }
  if (dlogits != nullptr) {
    const float g = (gout != nullptr ? gout[0] : 1.f) / (float)N, inv = 1.f / s;
    float* drow = dlogits + n * K;
    for (int k = threadIdx.x; k < K; k += blockDim.x)
      drow[k] = ok ? g * (expf(row[k] - m) * inv - (k == lab ? 1.f : 0.f)) : NAN;
  }
}
extern "C" int csmae_softmax_ce(long long N, int K, const float* logits, const long long* labels, const float* gout, float* scratch, float* loss, float* dlogits,
                                float* counts, int accumulate_counts, void* stream) {
  CSMAE_REQUIRE(N > 0 && N <= 0x7fffffffLL && K > 0 && logits && labels && scratch && loss, "csmae_softmax_ce: null or empty argument (scratch: 3 N floats)");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(softmax_ce_rows_kernel, dim3((unsigned)N), dim3(256), 0, st, N, K, logits, labels, gout, scratch, dlogits);
  hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(256), 0, st, N, 3, scratch, loss, counts, accumulate_counts);
  return csmae_check_launch("csmae_softmax_ce");
}
// Soft-target cross-entropy: loss = mean_n sum_k -t[n, k] log_softmax(z)[n, k], dlogits = gout (softmax sum_k t - t) / N.  The row's loss is
// summed as t ((m - z) + log s): non-negative terms, no cancellation against the row maximum m.  Row losses go to scratch [N].  V = 4: rows of
// K % 4 == 0 floats, 16-byte accesses.
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
    ldv<float, V>(row + k, z);
#pragma unroll
    for (int j = 0; j < V; ++j) m = fmaxf(m, z[j]);
  }
  m = block_max(m, red);
  float s = 0.f, ts = 0.f, a = 0.f;
  for (int k = threadIdx.x * V; k < K; k += blockDim.x * V) {
    float z[V], t[V];
    ldv<float, V>(row + k, z);
    ldv<float, V>(trow + k, t);
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
      ldv<float, V>(row + k, z);
      ldv<float, V>(trow + k, t);
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = g * (expf(z[j] - m) * inv - t[j]);
      stv<float, V>(drow + k, o);
    }
  }
}
extern "C" int csmae_soft_ce(long long N, int K, const float* logits, const float* target, const float* gout, float* scratch, float* loss, float* dlogits,
                             void* stream) {
  CSMAE_REQUIRE(N > 0 && N <= 0x7fffffffLL && K > 0 && logits && target && scratch && loss, "csmae_soft_ce: null or empty argument (scratch: N floats)");
  hipStream_t st = (hipStream_t)stream;
  if (vec4_ok(K, logits, target, dlogits)) hipLaunchKernelGGL(soft_ce_rows_kernel<4>, dim3((unsigned)N), dim3(256), 0, st, N, K, logits, target, gout, scratch, dlogits);
  else hipLaunchKernelGGL(soft_ce_rows_kernel<1>, dim3((unsigned)N), dim3(256), 0, st, N, K, logits, target, gout, scratch, dlogits);
  hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(256), 0, st, N, 1, scratch, loss, (float*)nullptr, 0);
  return csmae_check_launch("csmae_soft_ce");
}

// ---- classifier, backward.  dW / db: a thread owns one feature column d and HB_K consecutive classes, and walks the batch (x[n, d] coalesced
// over the workgroup, dlogits[n, k] uniform).  The workgroups of column block 0 also fold their classes' bias gradients, one wave per class.
// gscale: nullable device scalar (the upstream gradient of the loss) multiplied into both results.
#define HB_K 4
__global__ __launch_bounds__(256) void head_linear_bwd_kernel(long long N, int D, int K, const float* __restrict__ dl, const float* __restrict__ x,
                                                              const float* __restrict__ gscale, float* __restrict__ dw, float* __restrict__ db, int accumulate) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  const int k0 = blockIdx.y * HB_K;
  const int nk = min(HB_K, K - k0);
  const float g = gscale != nullptr ? gscale[0] : 1.f;
  if (d < D) {
    float s[HB_K];
#pragma unroll
    for (int j = 0; j < HB_K; ++j) s[j] = 0.f;
    for (long long n = 0; n < N; ++n) {
      const float xv = x[n * D + d];
#pragma unroll
      for (int j = 0; j < HB_K; ++j)
        if (j < nk) s[j] = fmaf(dl[n * K + k0 + j], xv, s[j]);
    }
#pragma unroll
    for (int j = 0; j < HB_K; ++j)
      if (j < nk) {
        float* o = dw + (long long)(k0 + j) * D + d;
        *o = accumulate ? *o + g * s[j] : g * s[j];
      }
  }
  if (blockIdx.x == 0 && db != nullptr) {
    const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;   // 4 waves = HB_K classes
    if (j < nk) {
      float s = 0.f;
      for (long long n = lane; n < N; n += 64) s += dl[n * K + k0 + j];
      s = wave_sum(s);
      if (lane == 0) db[k0 + j] = accumulate ? db[k0 + j] + g * s : g * s;
    }
  }
}
extern "C" int csmae_head_linear_bwd(long long N, int D, int K, const float* dlogits, const float* x, const float* gscale, float* dw, float* db, int accumulate,
                                     void* stream) {
  CSMAE_REQUIRE(N > 0 && D > 0 && K > 0 && dlogits && x && dw, "csmae_head_linear_bwd: null or empty argument");
  CSMAE_REQUIRE(cdiv(K, HB_K) <= 65535, "csmae_head_linear_bwd: K = %d is beyond the grid", K);
  hipLaunchKernelGGL(head_linear_bwd_kernel, dim3(cdiv(D, 256), cdiv(K, HB_K)), dim3(256), 0, (hipStream_t)stream, N, D, K, dlogits, x, gscale, dw, db, accumulate);
  return csmae_check_launch("csmae_head_linear_bwd");
}
// dX: a thread owns one feature column d (rows of W coalesced over the workgroup), a workgroup HD_ROWS samples (dlogits[n, k] is uniform over the
// workgroup); the classes are walked in order.
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
    ldv<T, V>(dres + n * td + i0, v);
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] += v[j];
  }
  constexpr int W = V >= 4 ? 4 : 1;   // 16-byte reads / writes of the fp32 result (dpos is 16-byte aligned whenever V > 1)
#pragma unroll
  for (int j = 0; j < V; j += W) {
    if (accumulate) {
      float o[W];
      ldv<float, W>(dpos + i0 + j, o);
#pragma unroll
      for (int k = 0; k < W; ++k) s[j + k] += o[k];
    }
    stv<float, W>(dpos + i0 + j, s + j);
  }
}
extern "C" int csmae_pos_embed_grad(int dtype, long long N, int T, int D, const void* dres, float* dpos, int accumulate, void* stream) {
  CSMAE_REQUIRE(N > 0 && T > 0 && D > 0 && dres && dpos, "csmae_pos_embed_grad: null or empty argument");
  CSMAE_REQUIRE(dtype == CSMAE_F32 || dtype == CSMAE_BF16, "csmae_pos_embed_grad: bad dtype %d", dtype);
  const long long td = (long long)T * D;
  const bool v4 = vec4_ok(td, dres, dpos);
  CSMAE_REQUIRE(cdiv(td, 256) <= 0x7fffffff, "csmae_pos_embed_grad: T D = %lld is beyond the grid", td);
  hipStream_t st = (hipStream_t)stream;
#define PEG(TT, VV) hipLaunchKernelGGL((pos_embed_grad_kernel<TT, VV>), dim3(cdiv(td, 256 * VV)), dim3(256), 0, st, N, td, (const TT*)dres, dpos, accumulate)
  if (dtype == CSMAE_F32) { if (v4) PEG(float, 4); else PEG(float, 1); }
  else if (v4 && td % 8 == 0) PEG(bf16_t, 8);
  else if (v4) PEG(bf16_t, 4);
  else PEG(bf16_t, 1);
#undef PEG
  return csmae_check_launch("csmae_pos_embed_grad");
}

// ---- LARS (util/lars.py:27-57) over a table of tensors: table[t] = {p, g, mu (device addresses), numel, ndim > 1}.  Launch 1 leaves LARS_PARTS
// partial sums of |p|^2 and |g + wd p|^2 per matrix in norms [ntensors][LARS_PARTS][2]; launch 2 folds them (every workgroup in the same order),
// forms q = trust |p| / |dp| (1 when either norm is 0) and applies mu = momentum mu + dp, p -= lr mu.  Vectors (ndim <= 1) take dp = g: no
// weight decay, no rate scaling.  lr is a kernel argument; nothing is read back.  gate (nullable device scalar, as for csmae_adamw): a
// non-finite value skips the update as a whole.
#define LARS_PARTS 64
__global__ __launch_bounds__(256) void lars_norm_kernel(const long long* __restrict__ table, float wd, float* __restrict__ norms) {
  __shared__ float red[17];
  const long long* t = table + (long long)blockIdx.y * 5;
  float* out = norms + ((long long)blockIdx.y * LARS_PARTS + blockIdx.x) * 2;
  if (t[4] == 0) { if (threadIdx.x == 0) { out[0] = 0.f; out[1] = 0.f; } return; }
  const float* p = reinterpret_cast<const float*>(t[0]);
  const float* g = reinterpret_cast<const float*>(t[1]);
  const long long n = t[3];
  float sp = 0.f, sd = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)LARS_PARTS * blockDim.x) {
    const float pv = p[i], dv = fmaf(wd, pv, g[i]);
    sp = fmaf(pv, pv, sp);
    sd = fmaf(dv, dv, sd);
  }
  sp = block_sum(sp, red);
  sd = block_sum(sd, red);
  if (threadIdx.x == 0) { out[0] = sp; out[1] = sd; }
}
__global__ __launch_bounds__(256) void lars_apply_kernel(const long long* __restrict__ table, float lr, float wd, float momentum, float trust,
                                                         const float* __restrict__ norms, const float* __restrict__ gate) {
  if (gate != nullptr && !isfinite(gate[0])) return;
  const long long* t = table + (long long)blockIdx.y * 5;
  float* p = reinterpret_cast<float*>(t[0]);
  const float* g = reinterpret_cast<const float*>(t[1]);
  float* mu = reinterpret_cast<float*>(t[2]);
  const long long n = t[3];
  const bool matrix = t[4] != 0;
  float q = 1.f;
  if (matrix) {
    const float* part = norms + (long long)blockIdx.y * LARS_PARTS * 2;
    float sp = 0.f, sd = 0.f;
    for (int i = 0; i < LARS_PARTS; ++i) { sp += part[2 * i]; sd += part[2 * i + 1]; }
    const float pn = sqrtf(sp), un = sqrtf(sd);
    q = (pn > 0.f && un > 0.f) ? trust * pn / un : 1.f;
  }
  const float w = matrix ? wd : 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float pv = p[i];
    const float dp = q * fmaf(w, pv, g[i]);
    const float m = fmaf(momentum, mu[i], dp);
    mu[i] = m;
    p[i] = pv - lr * m;
  }
}
extern "C" int csmae_lars_step(int ntensors, const long long* table, float lr, float weight_decay, float momentum, float trust, float* norms, const float* gate,
                               void* stream) {
  CSMAE_REQUIRE(ntensors > 0 && ntensors <= 65535 && table && norms, "csmae_lars_step: null or empty argument (norms: ntensors x 128 floats)");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lars_norm_kernel, dim3(LARS_PARTS, ntensors), dim3(256), 0, st, table, weight_decay, norms);
  hipLaunchKernelGGL(lars_apply_kernel, dim3(LARS_PARTS, ntensors), dim3(256), 0, st, table, lr, weight_decay, momentum, trust, norms, gate);
  return csmae_check_launch("csmae_lars_step");
}
