// k-NN evaluation of the frozen encoder (main_knn.py, csmae_hip/knn.py): what runs behind the similarity GEMM of a nearest-neighbour search.
//   l2_normalize   dst[r] = src[r] / max(||src[r]||_2, eps), fp32 in, fp32 or bf16 out (the bank once, the queries per search)
//   knn_select     merges one fp32 similarity tile [Q, Bc] into each query's running best-k list — the hot kernel: it reads every similarity once
//   knn_vote       DINO's weighted vote over the k neighbours' labels, the five best classes, top-1 / top-5 hits
// One wave owns one row in all three; a workgroup is four independent waves (no LDS traffic between them, no barrier in the hot kernel).  No atomics,
// fixed orders: two runs give the same bits.
#include "common.h"

#define KNN_WAVES 4   // rows per 256-thread workgroup
// every row of a matrix starts on a 16-byte boundary
static inline bool vec4_rows(const void* p, long long ld) { return ld % 4 == 0 && ((uintptr_t)p & 15) == 0; }

// ---- rows of unit length.  Lanes stride the row (coalesced; any D, any ld), the squares are summed in fp32: lane partials in column order, then the wave
// tree.  A zero row stays zero (0 / eps).
template <typename TO>
__global__ __launch_bounds__(256) void l2_normalize_kernel(long long rows, int D, const float* __restrict__ src, long long ld, float eps, TO* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * KNN_WAVES + (threadIdx.x >> 6);
  if (r >= rows) return;   // (whole waves leave: no barrier follows)
  const float* x = src + r * ld;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) { const float v = x[d]; s = fmaf(v, v, s); }
  s = wave_sum(s);
  const float inv = 1.f / fmaxf(sqrtf(s), eps);
  TO* o = dst + r * D;
  for (int d = lane; d < D; d += 64) st_from_f32<TO>(o + d, x[d] * inv);
}
extern "C" int csmae_l2_normalize(int in_dtype, int out_dtype, long long rows, int D, const void* src, long long ld, float eps, void* dst, void* stream) {
  CSMAE_REQUIRE(rows > 0 && D > 0 && src && dst && src != dst, "csmae_l2_normalize: null, empty or aliased argument");
  CSMAE_REQUIRE(in_dtype == CSMAE_F32, "csmae_l2_normalize: the source is fp32 (in_dtype %d)", in_dtype);
  CSMAE_REQUIRE(out_dtype == CSMAE_F32 || out_dtype == CSMAE_BF16, "csmae_l2_normalize: bad out_dtype %d", out_dtype);
  CSMAE_REQUIRE(ld >= D && eps > 0.f, "csmae_l2_normalize: ld = %lld must cover D = %d, eps = %g must be positive", ld, D, (double)eps);
  CSMAE_REQUIRE(cdiv(rows, KNN_WAVES) <= 0x7fffffffLL, "csmae_l2_normalize: rows = %lld is beyond the grid", rows);
  const dim3 grid(cdiv(rows, KNN_WAVES)), block(64 * KNN_WAVES);
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == CSMAE_F32) hipLaunchKernelGGL(l2_normalize_kernel<float>, grid, block, 0, st, rows, D, (const float*)src, ld, eps, (float*)dst);
  else hipLaunchKernelGGL(l2_normalize_kernel<bf16_t>, grid, block, 0, st, rows, D, (const float*)src, ld, eps, (bf16_t*)dst);
  return csmae_check_launch("csmae_l2_normalize");
}

// ---- best-k selection.  A list is ordered by (similarity descending, bank index ascending): `knn_before(a, b)` is that total order.  An unused slot is
// (-inf, -1); the index compares as unsigned, so -1 comes after every bank row of the same similarity and a row whose similarity is -inf still
// displaces an unused slot.  (A NaN similarity compares false both ways and is never listed.)
__device__ __forceinline__ bool knn_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && (unsigned)ai < (unsigned)bi); }

// The wave's list lives in registers, entry j in lane j (lanes k .. 63 hold unused slots for good); `tv, ti` = entry k - 1, the one a newcomer has to
// come before.  Because the order is total, candidates may be offered in any order and tiles merged in any order: the list is always the k first
// of everything seen.
struct KnnList {
  float v; int i;      // this lane's entry
  float tv; int ti;    // the threshold entry (wave-uniform)
  int k, lane;
  // Offer one candidate per lane (`live` lanes only).  The common case — no lane comes before the threshold — is one compare and one ballot.  Otherwise
  // the takers are inserted one at a time, each re-tested against the threshold as it stands by then: its place is the number of entries before it
  // (the list is sorted, so those are lanes 0 .. pos - 1), the entries from there on move up one lane and the last falls off.  A row in which every
  // element is a taker (ascending similarities) costs one insertion per element: slow, and correct.
  __device__ __forceinline__ void offer(float cv, int ci, bool live) {
    unsigned long long takers = __builtin_amdgcn_ballot_w64(live && knn_before(cv, ci, tv, ti));
    while (takers) {
      const int src = __builtin_ctzll(takers);
      takers &= takers - 1;
      const float nv = __shfl(cv, src, 64);
      const int ni = __shfl(ci, src, 64);
      if (!knn_before(nv, ni, tv, ti)) continue;   // (wave-uniform: an earlier insertion of this round raised the threshold past it)
      const int pos = __builtin_popcountll(__builtin_amdgcn_ballot_w64(knn_before(v, i, nv, ni)));   // < k: the candidate comes before entry k - 1
      const float uv = __shfl_up(v, 1, 64);
      const int ui = __shfl_up(i, 1, 64);
      if (lane < k) {
        if (lane > pos) { v = uv; i = ui; }
        else if (lane == pos) { v = nv; i = ni; }
      }
      tv = __shfl(v, k - 1, 64);
      ti = __shfl(i, k - 1, 64);
    }
  }
};

// One wave per query row.  V = 4: the row is 16-byte aligned (host: sim 16-byte aligned, ld % 4 == 0) and is read as float4, KNN_UNROLL of them in flight per
// lane (the kernel is a pure stream over the tile: Q Bc floats read once, 2 k words per query read and written); the columns behind the last whole
// float4 are read one by one.  V = 1: any alignment, one float per lane.  Columns >= Bc are never read.
#define KNN_UNROLL 4
template <int V>
__global__ __launch_bounds__(256) void knn_select_kernel(long long Q, int Bc, int k, const float* __restrict__ sim, long long ld, int base, float* __restrict__ val,
                                                         int* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const long long q = (long long)blockIdx.x * KNN_WAVES + (threadIdx.x >> 6);
  if (q >= Q) return;   // (whole waves leave: no barrier follows)
  KnnList L;
  L.k = k; L.lane = lane;
  L.v = lane < k ? val[q * k + lane] : -INFINITY;
  L.i = lane < k ? idx[q * k + lane] : -1;
  L.tv = __shfl(L.v, k - 1, 64);
  L.ti = __shfl(L.i, k - 1, 64);
  const float* row = sim + q * ld;
  int c0 = 0;
  if constexpr (V == 4) {
    const int whole = Bc & ~3;
    constexpr int STEP = 64 * 4 * KNN_UNROLL;   // columns per iteration of the wave
    for (; c0 < whole; c0 += STEP) {
      f4_t x[KNN_UNROLL];
      bool in[KNN_UNROLL];
#pragma unroll
      for (int u = 0; u < KNN_UNROLL; ++u) {
        const int c = c0 + (u * 64 + lane) * 4;
        in[u] = c < whole;
        x[u] = in[u] ? *reinterpret_cast<const f4_t*>(row + c) : f4_t{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      }
      // one test for the lane's 16 values: an element can only be a taker when it is >= the threshold's similarity (or the list is not full yet)
      float m = fmaxf(fmaxf(x[0][0], x[0][1]), fmaxf(x[0][2], x[0][3]));
      bool any = in[0];
#pragma unroll
      for (int u = 1; u < KNN_UNROLL; ++u) { m = fmaxf(m, fmaxf(fmaxf(x[u][0], x[u][1]), fmaxf(x[u][2], x[u][3]))); any = any || in[u]; }
      if (__builtin_amdgcn_ballot_w64(any && (m >= L.tv || L.ti < 0)) == 0ull) continue;
#pragma unroll
      for (int u = 0; u < KNN_UNROLL; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) L.offer(x[u][e], base + c0 + (u * 64 + lane) * 4 + e, in[u]);
    }
    c0 = whole;
  }
  for (; c0 < Bc; c0 += 64) {
    const int c = c0 + lane;
    const bool live = c < Bc;
    L.offer(live ? row[c] : -INFINITY, base + c, live);
  }
  if (lane < k) { val[q * k + lane] = L.v; idx[q * k + lane] = L.i; }
}
extern "C" int csmae_knn_select(long long Q, int Bc, int k, const float* sim, long long ld, long long base, float* val, int* idx, void* stream) {
  CSMAE_REQUIRE(k >= 1 && k <= 64, "csmae_knn_select: k = %d must lie in [1, 64] (one lane of a wave per list entry)", k);
  CSMAE_REQUIRE(Q > 0 && Bc > 0 && sim && val && idx, "csmae_knn_select: null or empty argument");
  CSMAE_REQUIRE(ld >= Bc, "csmae_knn_select: ld = %lld must cover Bc = %d", ld, Bc);
  // (a lane forms its column's index before it knows the column is inside the tile: up to one wave step past the end must still be an int)
  CSMAE_REQUIRE(base >= 0 && base + Bc <= 0x7ffff000LL, "csmae_knn_select: bank rows %lld .. %lld do not fit the int32 index", base, base + Bc - 1);
  CSMAE_REQUIRE(cdiv(Q, KNN_WAVES) <= 0x7fffffffLL, "csmae_knn_select: Q = %lld is beyond the grid", Q);
  const dim3 grid(cdiv(Q, KNN_WAVES)), block(64 * KNN_WAVES);
  hipStream_t st = (hipStream_t)stream;
  if (vec4_rows(sim, ld)) hipLaunchKernelGGL(knn_select_kernel<4>, grid, block, 0, st, Q, Bc, k, sim, ld, (int)base, val, idx);
  else hipLaunchKernelGGL(knn_select_kernel<1>, grid, block, 0, st, Q, Bc, k, sim, ld, (int)base, val, idx);
  return csmae_check_launch("csmae_knn_select");
}

// ---- weighted vote (DINO eval_knn.py knn_classifier): votes[q, c] = sum_j [label(idx[q, j]) == c] exp(val[q, j] / T).  The wave's K votes sit in LDS;
// lane j reads neighbour j (its label through the bank index) and the k weights are added in list order by one lane, so the sum has one order.  Then five
// rounds of a wave arg-max over (vote descending, class ascending): a lane scans classes lane, lane + 64, ..., the winner is marked -1 in LDS (votes are
// >= 0).  Classes nobody voted for rank by class id behind the others.  hits[q] = {top-1, top-5}; a second one-workgroup launch folds them in query order.
#define KNN_VOTE_KMAX 2048   // classes: 4 waves x 8 KiB of LDS
__global__ __launch_bounds__(256) void knn_vote_kernel(long long Q, int k, int K, const float* __restrict__ val, const int* __restrict__ idx,
                                                       const long long* __restrict__ bank_labels, float inv_T, float* __restrict__ votes, int* __restrict__ top5) {
  __shared__ float sv_all[KNN_WAVES][KNN_VOTE_KMAX];
  const int lane = threadIdx.x & 63;
  float* sv = sv_all[threadIdx.x >> 6];
  const long long q = (long long)blockIdx.x * KNN_WAVES + (threadIdx.x >> 6);
  if (q >= Q) return;   // (whole waves leave; the LDS rows are per wave and no barrier follows)
  for (int c = lane; c < K; c += 64) sv[c] = 0.f;
  float w = 0.f;
  int lab = -1;
  if (lane < k) {
    const int i = idx[q * k + lane];
    if (i >= 0) {
      const long long l = bank_labels[i];
      if (l >= 0 && l < K) { lab = (int)l; w = expf(val[q * k + lane] * inv_T); }
    }
  }
  for (int j = 0; j < k; ++j) {   // (LDS accesses of one wave complete in program order)
    const int lj = __shfl(lab, j, 64);
    const float wj = __shfl(w, j, 64);
    if (lane == 0 && lj >= 0) sv[lj] += wj;
  }
  if (votes != nullptr)
    for (int c = lane; c < K; c += 64) votes[q * K + c] = sv[c];
  for (int r = 0; r < 5; ++r) {
    float bv = -1.f;
    int bc = 0x7fffffff;
    for (int c = lane; c < K; c += 64) {
      const float v = sv[c];
      if (v > bv) { bv = v; bc = c; }   // (ascending c: the first of equal votes stays)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oc = __shfl_xor(bc, o, 64);
      if (ov > bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
    }
    const bool found = bv >= 0.f;   // (fewer than five classes: the tail is -1)
    if (lane == 0) {
      top5[q * 5 + r] = found ? bc : -1;
      if (found) sv[bc] = -1.f;
    }
  }
}
__global__ __launch_bounds__(256) void knn_count_kernel(long long Q, int K, const int* __restrict__ top5, const long long* __restrict__ labels, float* __restrict__ counts,
                                                        int accumulate) {
  __shared__ float red[17];
  float h1 = 0.f, h5 = 0.f;
  for (long long q = threadIdx.x; q < Q; q += blockDim.x) {
    const long long l = labels[q];
    if (l < 0 || l >= K) continue;   // (a label outside [0, K) scores no hit — and must not match the -1 tail)
    const int* t = top5 + q * 5;
    h1 += t[0] == l ? 1.f : 0.f;
    h5 += (t[0] == l || t[1] == l || t[2] == l || t[3] == l || t[4] == l) ? 1.f : 0.f;
  }
  h1 = block_sum(h1, red);
  h5 = block_sum(h5, red);
  if (threadIdx.x == 0) {
    counts[0] = accumulate ? counts[0] + h1 : h1;
    counts[1] = accumulate ? counts[1] + h5 : h5;
  }
}
extern "C" int csmae_knn_vote(long long Q, int k, int K, const float* val, const int* idx, const long long* bank_labels, float inv_T, float* votes, int* top5,
                              float* counts, const long long* query_labels, int accumulate_counts, void* stream) {
  CSMAE_REQUIRE(k >= 1 && k <= 64, "csmae_knn_vote: k = %d must lie in [1, 64]", k);
  CSMAE_REQUIRE(Q > 0 && val && idx && bank_labels && top5, "csmae_knn_vote: null or empty argument (votes, counts and query_labels may be null)");
  CSMAE_REQUIRE(K >= 1 && K <= KNN_VOTE_KMAX, "csmae_knn_vote: K = %d must lie in [1, %d]", K, KNN_VOTE_KMAX);
  CSMAE_REQUIRE(query_labels == nullptr || counts != nullptr, "csmae_knn_vote: query_labels need counts");
  CSMAE_REQUIRE(cdiv(Q, KNN_WAVES) <= 0x7fffffffLL, "csmae_knn_vote: Q = %lld is beyond the grid", Q);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(knn_vote_kernel, dim3(cdiv(Q, KNN_WAVES)), dim3(64 * KNN_WAVES), 0, st, Q, k, K, val, idx, bank_labels, inv_T, votes, top5);
  if (query_labels != nullptr) hipLaunchKernelGGL(knn_count_kernel, dim3(1), dim3(256), 0, st, Q, K, top5, query_labels, counts, accumulate_counts);
  return csmae_check_launch("csmae_knn_vote");
}
