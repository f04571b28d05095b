// Linear probing of the frozen encoder (main_linprobe.py:515-525, models_vit.py:53-58, util/lars.py:27-57): everything behind the last
// transformer block.  All arithmetic is fp32; only the token stream the pooling kernel reads may be bf16.  The kernels are small and
// HBM- / latency-bound (N x D x K is three orders of magnitude below one trunk forward): plain fp32 with fp32 accumulation, no MFMA route.
//   probe_pool   mean over the patch tokens (or the cls token) + LayerNorm -> feat [N, D]
//   bn1d         BatchNorm1d(D, affine=False) over the batch axis of feat, running statistics in training mode
//   head_linear  logits = fbn W^T + b; dW = dlogits^T fbn, db = sum_n dlogits
//   softmax_ce   mean cross-entropy, dlogits, top-1 / top-5 counts
//   lars_step    LARS over a pointer table of tensors: partial squared norms, then the update
#include "common.h"
#include "probe_common.h"

// ---- pooling + final norm (the pooling walk and the row statistics: probe_common.h, shared with the fine-tune head's backward).
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
  if (dtype == CSMAE_F32) hipLaunchKernelGGL((probe_pool_kernel<float, 4>), grid, block, 0, st, T, D, t0, t1, (const float*)x, gamma, beta, eps, feat);
  else if (D % 8 == 0) hipLaunchKernelGGL((probe_pool_kernel<bf16_t, 8>), grid, block, 0, st, T, D, t0, t1, (const bf16_t*)x, gamma, beta, eps, feat);
  else hipLaunchKernelGGL((probe_pool_kernel<bf16_t, 4>), grid, block, 0, st, T, D, t0, t1, (const bf16_t*)x, gamma, beta, eps, feat);
  return csmae_check_launch("csmae_probe_pool_fwd");
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

// Backward: a thread owns one feature column d and HB_K consecutive classes, and walks the batch (x[n, d] coalesced over the workgroup, dlogits[n, k]
// uniform).  The workgroups of column block 0 also fold their classes' bias gradients, one wave per class.  gscale: nullable device scalar (the
// upstream gradient of the loss) multiplied into both results.
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

// ---- softmax cross-entropy (torch.nn.CrossEntropyLoss, mean) with its gradient and the top-1 / top-5 hit counts (timm `accuracy`).  One workgroup per
// row, stable form (row maximum subtracted); row results go to scratch [3][N] = {loss, top-1 hit, top-5 hit}, a one-workgroup launch folds them in a
// fixed order.  A row counts toward top-k when fewer than min(k, K) logits are strictly greater than the label's.  A label outside [0, K) indexes
// nothing: its row's loss and gradient are NaN and it scores no hit.
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
__global__ __launch_bounds__(256) void softmax_ce_finish_kernel(long long N, const float* __restrict__ scratch, float* __restrict__ loss, float* __restrict__ counts,
                                                                int accumulate_counts) {
  __shared__ float red[17];
  float s[3];
  for (int j = 0; j < 3; ++j) {
    float a = 0.f;
    for (long long n = threadIdx.x; n < N; n += blockDim.x) a += scratch[j * N + n];
    s[j] = block_sum(a, red);
  }
  if (threadIdx.x == 0) {
    loss[0] = s[0] / (float)N;
    if (counts != nullptr) {
      counts[0] = accumulate_counts ? counts[0] + s[1] : s[1];
      counts[1] = accumulate_counts ? counts[1] + s[2] : s[2];
    }
  }
}
extern "C" int csmae_softmax_ce(long long N, int K, const float* logits, const long long* labels, const float* gout, float* scratch, float* loss, float* dlogits,
                                float* counts, int accumulate_counts, void* stream) {
  CSMAE_REQUIRE(N > 0 && N <= 0x7fffffffLL && K > 0 && logits && labels && scratch && loss, "csmae_softmax_ce: null or empty argument (scratch: 3 N floats)");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(softmax_ce_rows_kernel, dim3((unsigned)N), dim3(256), 0, st, N, K, logits, labels, gout, scratch, dlogits);
  hipLaunchKernelGGL(softmax_ce_finish_kernel, dim3(1), dim3(256), 0, st, N, scratch, loss, counts, accumulate_counts);
  return csmae_check_launch("csmae_softmax_ce");
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
