// Streaming (flash-style) bf16 MFMA attention for sequences whose K and V do not fit in LDS next to each other: any T <= 8192, any
// head_dim <= 128 that is a multiple of 8 (buckets 32 / 64 / 96 / 128, zero padded).  Same conventions as the LDS-resident family in
// attention.hip — S^T = K Q^T so that a lane owns one query column, P goes from the accumulators straight into the next MFMA's B operand,
// transposed operands come from row-major LDS images through ds_read_b64_tr_b16 — but a workgroup owns ATTN_STREAM_OWN (128) rows of one
// (sample, head), each of its four waves two 16-row blocks of them held in registers, and the other side of the product arrives in tiles
// of ATTN_STREAM_TILE (64) rows through a double-buffered LDS image: the global loads of tile i + 1 are issued before the arithmetic on
// tile i and written to the other buffer after it (HeadStager's register-staged split), one workgroup barrier per tile.
//   forward          : owns query rows, streams K / V.  Online softmax: running maximum m and sum l per query (l in fp32 from the
//                      un-rounded p, P rounded to bf16 once), O rescaled by exp2(m_old - m_new) per tile — lane-local in this layout.
//                      Keys >= T are masked in the last tile only.
//   backward, dQ     : owns query rows (Q, dO fragments, lse and delta = rowsum(dO o O) in registers), streams K / V.
//   backward, dK, dV : owns key rows (K, V fragments in registers), streams Q / dO with the tile's lse and delta (recomputed per tile from
//                      `out` and `dout`: a few VALU operations per row, and csmae_attn_bwd needs no workspace).
// The two backward passes are two block ranges of ONE launch (so csmae_next_launch_event's event rides on the kernel that completes
// dqkv); S and dP are recomputed in each pass; every output element is written once, by one workgroup, in a fixed order: no atomics,
// two runs give the same bits.
// Chosen: 128 owned rows x 64-row tiles, 256 threads.  hipcc -O3, -Rpass-analysis=kernel-resource-usage (registers = VGPR + AGPR; no kernel
// uses scratch or spills; __launch_bounds__(256, 2) at head_dim <= 64, so at least two workgroups share a CU there; LDS admits four or more):
//   head_dim bucket        32        64        96        128
//   forward   registers    117       158       237       312      LDS 20 / 36 / 52 / 68 KiB
//   backward  registers    144       225       402       490      LDS 21 / 37 / 53 / 69 KiB
// Not done: an XCD-aware block remap (one head's blocks are neighbours in launch order, so they land on different L2s) and staging O
// through LDS for whole-row stores — neither was measured.
#include "attention_common.h"

constexpr int SOWN = ATTN_STREAM_OWN, STILE = ATTN_STREAM_TILE, SNF = STILE / 16;
static_assert(SOWN == 4 * 2 * 16 && STILE == 64, "four waves x two 16-row blocks; four 16-row fragments (two k-packed pairs) per streamed tile");

// sum of the eight bf16 products of two 16-byte chunks
__device__ __forceinline__ float dot8_bf16(uint4 a, uint4 b) {
  const unsigned aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    acc += __uint_as_float(aw[k] << 16) * __uint_as_float(bw[k] << 16) + __uint_as_float(aw[k] & 0xffff0000u) * __uint_as_float(bw[k] & 0xffff0000u);
  return acc;
}
// a wave's two 16-row blocks of one head's matrix as MFMA fragments, straight from global memory (rows >= T and columns >= hd: zero)
template <int KS>
__device__ __forceinline__ void load_own(uint4 (&dst)[2][KS], const bf16_t* src, long long row0, int r0, int ld, int col0, int T, int hd, int t, int g) {
#pragma unroll
  for (int bq = 0; bq < 2; ++bq)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int r = r0 + 16 * bq + t, col = ks * 32 + 8 * g;
      dst[bq][ks] = make_uint4(0, 0, 0, 0);
      if (r < T && col < hd) dst[bq][ks] = *reinterpret_cast<const uint4*>(src + (row0 + r) * ld + col0 + col);
    }
}

// ------------------------------------------------------------------------------------------ forward
template <int HD>
__global__ __launch_bounds__(256, HD <= 64 ? 2 : 1) void attn_fwd_stream(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, float* __restrict__ lse,
                                                                         int T, int H, int D, int hd, float scale, int nown) {
  constexpr int KS = HD / 32, DF = HD / 16, IMG = STILE * AttnLds<HD>::STRIDE;
  __shared__ __attribute__((aligned(16))) char smem[4 * IMG];   // [buffer][K, V]
  const int bh = blockIdx.x / nown, own = blockIdx.x - bh * nown;
  const int b = bh / H, h = bh - b * H;
  const long long row0 = (long long)b * T;
  const int ld = 3 * D;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, g = lane >> 4;
  const int q0 = own * SOWN + w * 32;          // this wave's queries: blocks q0 and q0 + 16
  HeadStager<HD, STILE, 256, 2> sg;
  sg.load(0, qkv, row0, ld, D + h * hd, T, hd); sg.load(1, qkv, row0, ld, 2 * D + h * hd, T, hd);
  uint4 qraw[2][KS];
  load_own<KS>(qraw, qkv, row0, q0, ld, h * hd, T, hd, t, g);
  sg.store(0, smem); sg.store(1, smem + IMG);
  __syncthreads();
  const float c2 = scale * LOG2E;
  const bool live = q0 < T;                    // (wave-uniform) a wave past the end of the sequence only helps staging
  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};   // m in the log2 domain, already scaled; l: this lane's share of the row sum
  f4_t o[2][DF];
#pragma unroll
  for (int bq = 0; bq < 2; ++bq)
#pragma unroll
    for (int df = 0; df < DF; ++df) o[bq][df] = f4_t{0.f, 0.f, 0.f, 0.f};
  const int nt = (T + STILE - 1) / STILE;
  for (int it = 0; it < nt; ++it) {
    const char* Ks = smem + (it & 1) * 2 * IMG;
    const char* Vs = Ks + IMG;
    const bool more = it + 1 < nt;
    if (more) {
      const int k1 = (it + 1) * STILE;
      sg.load(0, qkv, row0 + k1, ld, D + h * hd, T - k1, hd); sg.load(1, qkv, row0 + k1, ld, 2 * D + h * hd, T - k1, hd);
    }
    if (live) {
      f4_t s[2][SNF];
#pragma unroll
      for (int f = 0; f < SNF; ++f) {
        s[0][f] = f4_t{0.f, 0.f, 0.f, 0.f}; s[1][f] = f4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const s8_t kf = frag_rows<HD>(Ks, f * 16, ks, t, g);
#pragma unroll
          for (int bq = 0; bq < 2; ++bq) s[bq][f] = MFMA16(kf, __builtin_bit_cast(s8_t, qraw[bq][ks]), s[bq][f]);
        }
      }
      if (!more) {                             // keys >= T exist in the last tile only: key it*64 + f*16 + 4g + r is padding
        const int kthr = T - it * STILE - 4 * g;
#pragma unroll
        for (int bq = 0; bq < 2; ++bq)
#pragma unroll
          for (int f = 0; f < SNF; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[bq][f][r] = (f * 16 + r >= kthr) ? -INFINITY : s[bq][f][r];
      }
      s8_t fp[2][SNF / 2];
#pragma unroll
      for (int bq = 0; bq < 2; ++bq) {
        float mt = -INFINITY;
#pragma unroll
        for (int f = 0; f < SNF; ++f) mt = fmaxf(fmaxf(mt, fmaxf(s[bq][f][0], s[bq][f][1])), fmaxf(s[bq][f][2], s[bq][f][3]));
        const float mn = fmaxf(m[bq], xrow_max(mt) * c2);        // every tile holds a real key: mn is finite
        const float alpha = __builtin_amdgcn_exp2f(m[bq] - mn);  // (first tile: exp2(-inf) = 0 on zero accumulators)
        m[bq] = mn;
        float ps = 0.f;
#pragma unroll
        for (int f = 0; f < SNF; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) { const float p = __builtin_amdgcn_exp2f(fmaf(s[bq][f][r], c2, -mn)); s[bq][f][r] = p; ps += p; }
        l[bq] = fmaf(l[bq], alpha, ps);
#pragma unroll
        for (int df = 0; df < DF; ++df) o[bq][df] *= alpha;
#pragma unroll
        for (int s2 = 0; s2 < SNF / 2; ++s2) fp[bq][s2] = pack_pair(s[bq][2 * s2], s[bq][2 * s2 + 1]);
      }
#pragma unroll
      for (int df = 0; df < DF; ++df)
#pragma unroll
        for (int s2 = 0; s2 < SNF / 2; ++s2) {
          const s8_t vf = frag_cols_tr<HD>(Vs, 32 * s2, df * 16, t, g);
#pragma unroll
          for (int bq = 0; bq < 2; ++bq) o[bq][df] = MFMA16(vf, fp[bq][s2], o[bq][df]);
        }
    }
    if (more) { char* nb = smem + ((it + 1) & 1) * 2 * IMG; sg.store(0, nb); sg.store(1, nb + IMG); }
    __syncthreads();                           // tile it + 1 is visible; nobody reads tile it's buffer any more
  }
  if (!live) return;
#pragma unroll
  for (int bq = 0; bq < 2; ++bq) {
    const int q = q0 + 16 * bq + t;
    const float lt = xrow_sum(l[bq]);
    const float inv = 1.0f / lt;
    if (q < T) {
#pragma unroll
      for (int df = 0; df < DF; ++df) {
        const int d = df * 16 + 4 * g;
        if (d < hd) st4<bf16_t>(out + (row0 + q) * D + h * hd + d, o[bq][df] * inv);
      }
      if (g == 0) lse[((long long)b * H + h) * T + q] = (m[bq] + log2f(lt)) * LN2;
    }
  }
}

// ------------------------------------------------------------------------------------------ backward
// query pass: dQ of this wave's 32 queries
template <int HD>
__device__ __forceinline__ void bwd_stream_dq(char* smem, const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                                              const float* __restrict__ lse, bf16_t* __restrict__ dqkv, int T, int H, int D, int hd, float scale, int b, int h, int own) {
  constexpr int KS = HD / 32, DF = HD / 16, IMG = STILE * AttnLds<HD>::STRIDE;
  const long long row0 = (long long)b * T;
  const int ld = 3 * D;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, g = lane >> 4;
  const int q0 = own * SOWN + w * 32;
  HeadStager<HD, STILE, 256, 2> sg;
  sg.load(0, qkv, row0, ld, D + h * hd, T, hd); sg.load(1, qkv, row0, ld, 2 * D + h * hd, T, hd);
  uint4 qraw[2][KS], graw[2][KS];
  float l2[2], dl[2];                          // log2-domain lse (+inf on padded rows: p = 0) and delta of query q0 + 16 bq + t
  load_own<KS>(qraw, qkv, row0, q0, ld, h * hd, T, hd, t, g);
  load_own<KS>(graw, dout, row0, q0, D, h * hd, T, hd, t, g);
  {
    uint4 oraw[2][KS];
    load_own<KS>(oraw, out, row0, q0, D, h * hd, T, hd, t, g);
#pragma unroll
    for (int bq = 0; bq < 2; ++bq) {
      const int q = q0 + 16 * bq + t;
      l2[bq] = q < T ? lse[((long long)b * H + h) * T + q] * LOG2E : INFINITY;
      float acc = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc += dot8_bf16(oraw[bq][ks], graw[bq][ks]);
      dl[bq] = xrow_sum(acc);
    }
  }
  sg.store(0, smem); sg.store(1, smem + IMG);
  __syncthreads();
  const float c2 = scale * LOG2E;
  const bool live = q0 < T;
  f4_t dq[2][DF];
#pragma unroll
  for (int bq = 0; bq < 2; ++bq)
#pragma unroll
    for (int df = 0; df < DF; ++df) dq[bq][df] = f4_t{0.f, 0.f, 0.f, 0.f};
  const int nt = (T + STILE - 1) / STILE;
  for (int it = 0; it < nt; ++it) {
    const char* Ks = smem + (it & 1) * 2 * IMG;
    const char* Vs = Ks + IMG;
    const bool more = it + 1 < nt;
    if (more) {
      const int k1 = (it + 1) * STILE;
      sg.load(0, qkv, row0 + k1, ld, D + h * hd, T - k1, hd); sg.load(1, qkv, row0 + k1, ld, 2 * D + h * hd, T - k1, hd);
    }
    if (live) {
      s8_t fds[2][SNF / 2];
      f4_t prev[2];
#pragma unroll
      for (int f = 0; f < SNF; ++f) {
        f4_t a[2] = {f4_t{0.f, 0.f, 0.f, 0.f}, f4_t{0.f, 0.f, 0.f, 0.f}}, dp[2] = {f4_t{0.f, 0.f, 0.f, 0.f}, f4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const s8_t kf = frag_rows<HD>(Ks, f * 16, ks, t, g), vf = frag_rows<HD>(Vs, f * 16, ks, t, g);
#pragma unroll
          for (int bq = 0; bq < 2; ++bq) {
            a[bq] = MFMA16(kf, __builtin_bit_cast(s8_t, qraw[bq][ks]), a[bq]);
            dp[bq] = MFMA16(vf, __builtin_bit_cast(s8_t, graw[bq][ks]), dp[bq]);
          }
        }
        // no key masking: padded K rows are zero, so whatever dS holds for a padded key adds 0 to dQ
#pragma unroll
        for (int bq = 0; bq < 2; ++bq) {
          f4_t ds;
#pragma unroll
          for (int r = 0; r < 4; ++r) ds[r] = __builtin_amdgcn_exp2f(fmaf(a[bq][r], c2, -l2[bq])) * (dp[bq][r] - dl[bq]) * scale;
          if (f & 1) fds[bq][f >> 1] = pack_pair(prev[bq], ds); else prev[bq] = ds;
        }
      }
#pragma unroll
      for (int df = 0; df < DF; ++df)
#pragma unroll
        for (int s2 = 0; s2 < SNF / 2; ++s2) {
          const s8_t kT = frag_cols_tr<HD>(Ks, 32 * s2, df * 16, t, g);
#pragma unroll
          for (int bq = 0; bq < 2; ++bq) dq[bq][df] = MFMA16(kT, fds[bq][s2], dq[bq][df]);
        }
    }
    if (more) { char* nb = smem + ((it + 1) & 1) * 2 * IMG; sg.store(0, nb); sg.store(1, nb + IMG); }
    __syncthreads();
  }
  if (!live) return;
#pragma unroll
  for (int bq = 0; bq < 2; ++bq) {
    const int q = q0 + 16 * bq + t;
#pragma unroll
    for (int df = 0; df < DF; ++df) {
      const int d = df * 16 + 4 * g;
      if (q < T && d < hd) st4<bf16_t>(dqkv + (row0 + q) * ld + h * hd + d, dq[bq][df]);
    }
  }
}

// key pass: dK, dV of this wave's 32 keys
template <int HD>
__device__ __forceinline__ void bwd_stream_dkv(char* smem, const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                                               const float* __restrict__ lse, bf16_t* __restrict__ dqkv, int T, int H, int D, int hd, float scale, int b, int h, int own) {
  constexpr int KS = HD / 32, DF = HD / 16, IMG = STILE * AttnLds<HD>::STRIDE, CH = HD / 8, NC = (CH + 3) / 4;
  float* stats = reinterpret_cast<float*>(smem + 4 * IMG);   // [buffer][lse2, delta][STILE]
  const long long row0 = (long long)b * T;
  const int ld = 3 * D;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = lane & 15, g = lane >> 4;
  const int k0 = own * SOWN + w * 32;          // this wave's keys: blocks k0 and k0 + 16
  // the streamed tile's statistics: four threads per query row, each the 16-byte chunks part, part + 4, ... of the row
  const int srow = threadIdx.x >> 2, part = threadIdx.x & 3;
  HeadStager<HD, STILE, 256, 2> sg;
  uint4 ov[NC], gv[NC];
  float lraw;
  auto load_tile = [&](int i0) {
    sg.load(0, qkv, row0 + i0, ld, h * hd, T - i0, hd); sg.load(1, dout, row0 + i0, D, h * hd, T - i0, hd);
    const bool in = i0 + srow < T;
    lraw = in ? lse[((long long)b * H + h) * T + i0 + srow] * LOG2E : INFINITY;   // padded queries: p = exp2(-inf) = 0
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int c = part + 4 * i;
      ov[i] = make_uint4(0, 0, 0, 0); gv[i] = make_uint4(0, 0, 0, 0);
      if (in && c < CH && c * 8 < hd) {
        ov[i] = *reinterpret_cast<const uint4*>(out + (row0 + i0 + srow) * D + h * hd + c * 8);
        gv[i] = *reinterpret_cast<const uint4*>(dout + (row0 + i0 + srow) * D + h * hd + c * 8);
      }
    }
  };
  auto store_tile = [&](int buf) {
    sg.store(0, smem + buf * 2 * IMG); sg.store(1, smem + buf * 2 * IMG + IMG);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) acc += dot8_bf16(ov[i], gv[i]);
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    if (part == 0) { stats[buf * 2 * STILE + srow] = lraw; stats[buf * 2 * STILE + STILE + srow] = acc; }
  };
  load_tile(0);
  uint4 kraw[2][KS], vraw[2][KS];
  load_own<KS>(kraw, qkv, row0, k0, ld, D + h * hd, T, hd, t, g);
  load_own<KS>(vraw, qkv, row0, k0, ld, 2 * D + h * hd, T, hd, t, g);
  store_tile(0);
  __syncthreads();
  const float c2 = scale * LOG2E;
  const bool live = k0 < T;
  f4_t dk[2][DF], dv[2][DF];
#pragma unroll
  for (int bk = 0; bk < 2; ++bk)
#pragma unroll
    for (int df = 0; df < DF; ++df) { dk[bk][df] = f4_t{0.f, 0.f, 0.f, 0.f}; dv[bk][df] = f4_t{0.f, 0.f, 0.f, 0.f}; }
  const int nt = (T + STILE - 1) / STILE;
  for (int it = 0; it < nt; ++it) {
    const char* Qs = smem + (it & 1) * 2 * IMG;
    const char* Gs = Qs + IMG;                 // dO
    const float* st = stats + (it & 1) * 2 * STILE;
    const bool more = it + 1 < nt;
    if (more) load_tile((it + 1) * STILE);
    if (live) {
      // per pair of query fragments (32 queries = one k-packed operand): S, dP -> P, dS -> their contribution to dK, dV
#pragma unroll
      for (int s2 = 0; s2 < SNF / 2; ++s2) {
        s8_t fp[2], fds[2];
        f4_t prev_p[2], prev_ds[2];
#pragma unroll
        for (int f = 2 * s2; f < 2 * s2 + 2; ++f) {
          f4_t a[2] = {f4_t{0.f, 0.f, 0.f, 0.f}, f4_t{0.f, 0.f, 0.f, 0.f}}, dp[2] = {f4_t{0.f, 0.f, 0.f, 0.f}, f4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const s8_t qf = frag_rows<HD>(Qs, f * 16, ks, t, g), gf = frag_rows<HD>(Gs, f * 16, ks, t, g);
#pragma unroll
            for (int bk = 0; bk < 2; ++bk) {
              a[bk] = MFMA16(qf, __builtin_bit_cast(s8_t, kraw[bk][ks]), a[bk]);
              dp[bk] = MFMA16(gf, __builtin_bit_cast(s8_t, vraw[bk][ks]), dp[bk]);
            }
          }
          const f4_t l4 = *reinterpret_cast<const f4_t*>(st + f * 16 + 4 * g);
          const f4_t d4 = *reinterpret_cast<const f4_t*>(st + STILE + f * 16 + 4 * g);
#pragma unroll
          for (int bk = 0; bk < 2; ++bk) {
            f4_t p, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              p[r] = __builtin_amdgcn_exp2f(fmaf(a[bk][r], c2, -l4[r]));
              ds[r] = p[r] * (dp[bk][r] - d4[r]) * scale;
            }
            if (f & 1) { fp[bk] = pack_pair(prev_p[bk], p); fds[bk] = pack_pair(prev_ds[bk], ds); } else { prev_p[bk] = p; prev_ds[bk] = ds; }
          }
        }
#pragma unroll
        for (int df = 0; df < DF; ++df) {
          const s8_t qT = frag_cols_tr<HD>(Qs, 32 * s2, df * 16, t, g), gT = frag_cols_tr<HD>(Gs, 32 * s2, df * 16, t, g);
#pragma unroll
          for (int bk = 0; bk < 2; ++bk) {
            dk[bk][df] = MFMA16(qT, fds[bk], dk[bk][df]);
            dv[bk][df] = MFMA16(gT, fp[bk], dv[bk][df]);
          }
        }
      }
    }
    if (more) store_tile((it + 1) & 1);
    __syncthreads();
  }
  if (!live) return;
#pragma unroll
  for (int bk = 0; bk < 2; ++bk) {
    const int key = k0 + 16 * bk + t;
#pragma unroll
    for (int df = 0; df < DF; ++df) {
      const int d = df * 16 + 4 * g;
      if (key < T && d < hd) {
        st4<bf16_t>(dqkv + (row0 + key) * ld + D + h * hd + d, dk[bk][df]);
        st4<bf16_t>(dqkv + (row0 + key) * ld + 2 * D + h * hd + d, dv[bk][df]);
      }
    }
  }
}

// one launch, two block ranges per (sample, head): blocks [0, nown) of a head are its query pass, [nown, 2 nown) its key pass
template <int HD>
__global__ __launch_bounds__(256, HD <= 64 ? 2 : 1) void attn_bwd_stream(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                                                                         const float* __restrict__ lse, bf16_t* __restrict__ dqkv, int T, int H, int D, int hd,
                                                                         float scale, int nown) {
  __shared__ __attribute__((aligned(16))) char smem[4 * STILE * AttnLds<HD>::STRIDE + 4 * STILE * 4];
  const int bh = blockIdx.x / (2 * nown), r = blockIdx.x - bh * 2 * nown;
  const int b = bh / H, h = bh - b * H;
  if (r < nown) bwd_stream_dq<HD>(smem, qkv, out, dout, lse, dqkv, T, H, D, hd, scale, b, h, r);
  else bwd_stream_dkv<HD>(smem, qkv, out, dout, lse, dqkv, T, H, D, hd, scale, b, h, r - nown);
}

// ------------------------------------------------------------------------------------------ launch
// A grid holds 2^32 threads at most: 2^24 - 1 workgroups of 256.
static int stream_blocks(const char* who, long long B, int T, int H, int per_own, int* nown, unsigned* nblk) {
  *nown = cdiv(T, SOWN);
  const long long n = B * H * *nown * per_own;
  CSMAE_REQUIRE(n <= 0xffffffll, "%s: B x H x ceil(T / %d) = %lld workgroups exceed one grid (streaming kernels)", who, SOWN, n);
  *nblk = (unsigned)n;
  return CSMAE_OK;
}
#define STREAM_BUCKETS(CALL) if (hd <= 32) { CALL(32); } else if (hd <= 64) { CALL(64); } else if (hd <= 96) { CALL(96); } else { CALL(128); }

int attn_stream_fwd(long long B, int T, int H, int hd, const void* qkv, void* out, float* lse, hipStream_t st) {
  int nown; unsigned nblk;
  if (int rc = stream_blocks("csmae_attn_fwd", B, T, H, 1, &nown, &nblk)) return rc;
  const int D = H * hd;
  const float scale = 1.0f / sqrtf((float)hd);
#define CALL(HDV) hipLaunchKernelGGL((attn_fwd_stream<HDV>), dim3(nblk), dim3(256), 0, st, (const bf16_t*)qkv, (bf16_t*)out, lse, T, H, D, hd, scale, nown)
  STREAM_BUCKETS(CALL)
#undef CALL
  return CSMAE_OK;
}

int attn_stream_bwd(long long B, int T, int H, int hd, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, hipStream_t st) {
  int nown; unsigned nblk;
  if (int rc = stream_blocks("csmae_attn_bwd", B, T, H, 2, &nown, &nblk)) return rc;
  const int D = H * hd;
  const float scale = 1.0f / sqrtf((float)hd);
#define CALL(HDV) CSMAE_LAUNCH((attn_bwd_stream<HDV>), dim3(nblk), dim3(256), 0, st, (const bf16_t*)qkv, (const bf16_t*)out, (const bf16_t*)dout, lse, (bf16_t*)dqkv, T, H, D, hd, scale, nown)
  STREAM_BUCKETS(CALL)
#undef CALL
  return CSMAE_OK;
}
