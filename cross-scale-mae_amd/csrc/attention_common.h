// Operand helpers shared by the bf16 MFMA attention kernels: the LDS-resident family (attention.hip) and the streaming family
// (attention_stream.hip).  Everything is computed TRANSPOSED (S^T = K Q^T): see the head of attention.hip.
#pragma once
#include "common.h"

#define LOG2E 1.4426950408889634f
#define LN2 0.6931471805599453f

// ------------------------------------------------------------------------------------------ bf16 helpers
template <int HD> struct AttnLds { static constexpr int STRIDE = (HD + 8) * 2; };  // bytes per row (16-B multiple)

// stage rows [0,TP) of one head's matrix (column offset `col0` inside a [B*T, ld] tensor) into LDS, zero padded
template <int HD, int TP>
__device__ __forceinline__ void stage_head(char* dst, const bf16_t* src, long long row0, int ld, int col0, int T, int hd) {
  constexpr int CH = HD / 8;
  for (int e = threadIdx.x; e < TP * CH; e += blockDim.x) {
    int r = e / CH, c = e - r * CH;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < T && c * 8 < hd) v = *reinterpret_cast<const uint4*>(src + (row0 + r) * ld + col0 + c * 8);
    *reinterpret_cast<uint4*>(dst + r * AttnLds<HD>::STRIDE + c * 16) = v;
  }
}

// The same for several matrices at once, with every global load issued before the first LDS store.  stage_head() called three or
// four times in a row ran ~3.5 dependent load->store iterations per matrix: ~10 exposed memory latencies (~10 of the ~18 us a
// workgroup lives) before any arithmetic could start.
template <int HD, int TP, int NT, int NM>
struct HeadStager {
  static constexpr int CH = HD / 8, IT = (TP * CH + NT - 1) / NT;
  uint4 v[NM][IT];
  __device__ __forceinline__ void load(int m, const bf16_t* src, long long row0, int ld, int col0, int T, int hd) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int e = threadIdx.x + i * NT, r = e / CH, c = e - r * CH;
      v[m][i] = make_uint4(0, 0, 0, 0);
      if (e < TP * CH && r < T && c * 8 < hd) v[m][i] = *reinterpret_cast<const uint4*>(src + (row0 + r) * ld + col0 + c * 8);
    }
  }
  __device__ __forceinline__ void store(int m, char* dst) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int e = threadIdx.x + i * NT, r = e / CH, c = e - r * CH;
      if (e < TP * CH) *reinterpret_cast<uint4*>(dst + r * AttnLds<HD>::STRIDE + c * 16) = v[m][i];
    }
  }
};

// K-contiguous fragment (lane (t,g): row = row0 + t, elements d = ks*32 + 8g .. +8)
template <int HD>
__device__ __forceinline__ s8_t frag_rows(const char* img, int row0, int ks, int t, int g) {
  return *reinterpret_cast<const s8_t*>(img + (row0 + t) * AttnLds<HD>::STRIDE + (ks * 32 + 8 * g) * 2);
}
// transposed fragment via tr-read: A operand with i = column (c0 + t) and k = rows {r0+4g+j, r0+16+4g+j}
template <int HD>
__device__ __forceinline__ s8_t frag_cols_tr(const char* img, int r0, int c0, int t, int g) {
  const char* p = img + (r0 + 4 * g + (t >> 2)) * AttnLds<HD>::STRIDE + (c0 + (t & 3) * 4) * 2;
  s4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s4_t, p));
  s4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s4_t, p + 16 * AttnLds<HD>::STRIDE));
  return join_s4(lo, hi);
}
__device__ __forceinline__ s8_t pack_pair(f4_t a, f4_t b) {
  unsigned u0 = pack2bf(a[0], a[1]), u1 = pack2bf(a[2], a[3]), u2 = pack2bf(b[0], b[1]), u3 = pack2bf(b[2], b[3]);
  uint4 u = make_uint4(u0, u1, u2, u3);
  return __builtin_bit_cast(s8_t, u);
}
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8_t, a), __builtin_bit_cast(bf8_t, b), c, 0, 0, 0)

// ------------------------------------------------------------------------------------------ streaming family (attention_stream.hip)
// rows a workgroup owns (query rows in the forward and the dQ pass, key rows in the dK / dV pass) and rows of one streamed tile
#define ATTN_STREAM_OWN 128
#define ATTN_STREAM_TILE 64
// launch only (the caller checks geometry and runs csmae_check_launch): CSMAE_OK, or CSMAE_ERR_ARG with the error text set
int attn_stream_fwd(long long B, int T, int H, int hd, const void* qkv, void* out, float* lse, hipStream_t st);
int attn_stream_bwd(long long B, int T, int H, int hd, const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, hipStream_t st);
