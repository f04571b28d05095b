/* libcsmae_hip — C ABI of the MI355X (gfx950) Cross-Scale MAE pre-training hot path.
 *
 * The reference (aicip/Cross-Scale-MAE) is pure Python and has NO native/FFI boundary of its own
 * (SURVEY §8b): its "operators" are ATen/timm calls inside the Python files of `models_mae/` and `engine_pretrain.py`.
 * Each entry point below therefore cites the reference expression it replaces (paths relative to the
 * reference root) rather than a pre-existing FFI symbol.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous memory owned by the caller (PyTorch allocates);
 *     kernels never allocate, free or retain pointers;
 *   - `stream` is a hipStream_t; calls only enqueue work and return immediately (no implicit sync);
 *   - return 0 on success, negative csmae_status otherwise; csmae_last_error() gives a thread-local text;
 *   - dtype: CSMAE_F32 = 0 (exact-fp32 parity mode), CSMAE_BF16 = 1 (MFMA throughput mode; raw bf16 bits);
 *   - row "views": storage_row(r) = (r / group) * gstride + off + r % group  (the `[:, 1:, :]` slices);
 *   - scalars that change every step (crop box, upstream gradient, AdamW hyper-parameters) are read from
 *     device memory so a captured hipGraph of the step stays valid.
 */
#ifndef CSMAE_H
#define CSMAE_H
#ifdef __cplusplus
extern "C" {
#endif

#define CSMAE_F32 0
#define CSMAE_BF16 1

enum csmae_status { CSMAE_OK = 0, CSMAE_ERR_ARG = -1, CSMAE_ERR_LAUNCH = -2, CSMAE_ERR_UNSUPPORTED = -3 };
enum csmae_epilogue { CSMAE_EPI_NONE = 0, CSMAE_EPI_GELU = 1, CSMAE_EPI_RESID = 2, CSMAE_EPI_DGELU = 3, CSMAE_EPI_ATOMIC = 4, CSMAE_EPI_SPLIT = 5,
                      CSMAE_EPI_GELU_Q8 = 6, CSMAE_EPI_DGELU_Q8 = 7 /* bf16 path: aux = gelu'(x) as one byte per element, q = round(200 g + 26): g = 0 and 1 are codes 26 and 226 exactly */ };
enum csmae_loss { CSMAE_LOSS_MSE = 0, CSMAE_LOSS_L2 = 1, CSMAE_LOSS_MAE = 2, CSMAE_LOSS_L1 = 3, CSMAE_LOSS_BCE = 4 };

const char* csmae_last_error(void);
int csmae_abi_version(void);
const char* csmae_source_hash(void);   /* sha256 of the kernel sources the library was built from (tools/csrc_hash.py): profiles are keyed to it */

/* ---- completion event of the NEXT kernel launch of the calling host thread (ABI version 4).  The reference hands work between streams through
 * events that torch records BEHIND a kernel (autograd's stream hand-offs; DistributedDataParallel's bucket hooks, main_pretrain.py:417-421);
 * a recorded event is a marker packet that costs the recording stream 3-5 us.  csmae_next_launch_event(ev) makes the next csmae_gemm /
 * csmae_gemm_fp8 (pipelined kernels) / csmae_attn_bwd (bf16) launch carry `ev` (a hipEvent_t) as its dispatch packet's completion signal
 * instead; csmae_flush_launch_event(stream) records it the plain way when that launch did not take it (other kernels), nullptr clears it.  */
int csmae_next_launch_event(void* hip_event);
int csmae_flush_launch_event(void* stream);

/* ---- dense contractions: nn.Linear of timm Block / decoder_embed / decoder_pred / predictor and their backward
 * (timm 0.4.12 Attention.qkv/.proj, Mlp.fc1/.fc2 — call sites models_mae/MAE_ViT_Baseline.py:160-188,270,295;
 *  models_mae/MLP.py:6,9).  C[M,N] = sum_k A(m,k) B(k,n); transX = 0: K contiguous ([M,K] / [N,K]); 1: K strided ([K,M] / [K,N]).
 *  epilogue: NONE (+bias) | GELU (x = acc + bias: C = gelu(x), aux = gelu'(x)) | RESID (C = acc + bias + resid; both in c_dtype:
 *            the fp32 residual stream, or the bf16 one of throughput mode) |
 *            DGELU (C = acc * aux) | ATOMIC (fp32 C += acc) | SPLIT (fp32 split-K slabs, see csmae_gemm_dw). */
int csmae_gemm(int dtype, int transA, int transB, long long M, long long N, long long K,
               const void* A, long long lda, const void* B, long long ldb, void* C, long long ldc, int c_dtype,
               const float* bias, int epilogue, void* aux, long long ldaux, const void* resid /* in C's dtype */, long long ldr,
               int splitk, void* stream);

/* ---- the same forward product y = x W^T (+ epilogue) with the weight given as its K-SLAB mirror (ABI version 6): Wk[K/32][slab_rows][32] bf16,
 * Wk[(k / 32) * slab_rows * 32 + n * 32 + k % 32] = W[n][k] — written by csmae_weights_kslab from the bf16 weight mirror after every optimizer
 * step.  Rows of a slab are 64 B, so 16 consecutive rows of one 32-wide K half are 1 KiB contiguous: the 128 x 256-tile kernel that runs TWO
 * 4-wave workgroups per CU (one's C-tile stores run under the other's MFMA loop) stages its weight operand per wave and per K half in whole
 * cache lines (csrc/gemm_k2.hip).  `B_plain` ([N][K], torch's layout) is used for the shapes that kernel does not take (K % 64 != 0, M < 128,
 * N < 256, fp32): same results either way (same MFMA shape and K order: bit-identical to csmae_gemm).  The dX products (transB = 1) reach the
 * same kernel through csmae_gemm: W[K][N] is K-strided with 128-B row segments per wave by nature.  csmae_gemm_k2_mode(nn, nt) switches the
 * two uses off / on (A/B aid, default on).  timm Block call sites: MAE_ViT_Baseline.py:160-188. */
int csmae_gemm_ks(int dtype, long long M, long long N, long long K, const void* A, long long lda, const void* Bk, long long slab_rows,
                  const void* B_plain, long long ldb_plain, void* C, long long ldc, int c_dtype, const float* bias, int epilogue,
                  void* aux, long long ldaux, const void* resid, long long ldr, void* stream);
/* desc: device int64 [count][3] = {offset (elements) of weight i in src AND dst, out-features N, in-features K (K % 64 == 0)}; one launch of
 * (max_blocks, count) workgroups */
int csmae_weights_kslab(int count, const long long* desc, int max_blocks, const void* src_bf16, void* dst_bf16, void* stream);
/* ---- a Linear product of timm's Block WITH the LayerNorm next to it in its epilogue (ABI version 7; csrc/gemm_ln.hip): a 128 x 512 tile — eight
 * waves side by side along N, one workgroup per CU — holds whole output rows (N <= 512, N % 64 == 0: the decoders), so the row statistics are made
 * inside the workgroup.  All tensors bf16 (the throughput mode's residual stream); bias / gamma / beta / mean / rstd fp32; K % 64 == 0.
 *   fwd  X = A Wk^T + bias + resid ; Y = LayerNorm(X; gamma, beta, eps) ; mean / rstd of X          [Wk: the K-slab mirror, as csmae_gemm_ks]
 *        = `x = x + attn.proj(..)` -> `norm2(x)`, and `x = x + mlp.fc2(..)` -> the NEXT block's `norm1(x)`     (MAE_ViT_Baseline.py:160-188)
 *   bwd  dx_out = LayerNorm'(dY W; x, mean, rstd, gamma) + dres_in ; partial_ws[ceil(M / 128)][2][N] = the tiles' dgamma / dbeta rows
 *        (W [K][N] as torch stores the layer's weight, K = out-features) = the backward of `norm2 -> mlp.fc1` and `norm1 -> attn.qkv`; the
 *        product itself never reaches HBM.  Same arithmetic as csmae_gemm + csmae_layernorm_bwd on the bf16-rounded product; fixed summation
 *        order (bit-reproducible).  csmae_ln_param_reduce_rows folds the partial rows (rows = ceil(M / 128)). */
int csmae_gemm_ln_supported(long long M, long long N, long long K);
int csmae_gemm_ln_fwd(long long M, long long N, long long K, const void* A, long long lda, const void* Bk, long long slab_rows,
                      const float* bias, const void* resid, long long ldr, void* X, long long ldx, const float* gamma, const float* beta,
                      float eps, void* Y, long long ldy, float* mean, float* rstd, void* stream);
int csmae_gemm_ln_bwd(long long M, long long N, long long K, const void* dY, long long lda, const void* W, long long ldb,
                      const void* x, long long ldx, const float* mean, const float* rstd, const float* gamma, const void* dres_in, long long ldd,
                      void* dx_out, long long ldo, float* partial_ws, long long partial_elems, void* stream);
int csmae_gemm_k2_mode(int nn, int nt);
int csmae_gemm_dw_mode(int k2);   /* csmae_gemm_dw_group on the 256 x 256 one-workgroup kernel (0, default) or the two-workgroups-per-CU one (1): measured slower in the step, kept as an option */

/* weight gradient of nn.Linear: dW[M=out,N=in] (fp32, contiguous) += dY[K,M]^T X[K,N]; token axis split over the chip into fp32 slabs in
 * `workspace` (>= M*N+M floats; more = more slices), folded by a deterministic reduce; db[M] (nullable) += column sums of dY, computed
 * inside the same kernel by an all-ones MFMA operand (util/misc.py:314 backward products). */
int csmae_gemm_dw(int dtype, long long M, long long N, long long K, const void* dY, long long ldy, const void* X, long long ldx,
                  float* dW, float* db, float* workspace, long long ws_elems, void* stream);
/* The weight gradients of several nn.Linear layers that reduce over the same K tokens (a transformer block's qkv / proj / fc1 / fc2:
 * MAE_ViT_Baseline.py:160-188 backward) in ONE launch: host arrays of `count` (<= 8) device pointers / sizes.  Together the products
 * fill `slots` workgroups (<= 0: 128) with no or few K slices.  One slice: the tile is accumulated into dW / db directly; several: dense
 * fp32 slabs + one ordered fold for the whole group (bit-reproducible either way).  workspace: >= tiles * slices * 65 792 floats (less
 * = fewer slices).  fp32 parity mode and products with M or N < 256 are run one by one through csmae_gemm_dw. */
int csmae_gemm_dw_group(int dtype, int count, long long K, const void* const* dY, const long long* ldy, const void* const* X,
                        const long long* ldx, float* const* dW, float* const* db, const long long* M, const long long* N, int slots,
                        float* workspace, long long ws_elems, void* stream);
/* The same grouped weight gradients with fp8 operands (ABI version 7; BASELINE.json configs[4]; csrc/gemm_fp8_dw.hip): dW[i] += dq_y[i] dq_x[i] dY8[i]^T X8[i],
 * db[i] (nullable) += dq_y[i] colsum(dY8[i]); dY8 e5m2 bytes [K][ldy] (the gradient copies the dX products read), X8 e4m3 bytes [K][ldx] (the activation
 * copies the forward products read), dq_* device scalars (the de-quantisation factors their producers left), fp32 accumulation on
 * v_mfma_scale_f32_16x16x128_f8f6f4 with both operands K-strided (ds_read_b64_tr_b8).  M, N >= 256, N % 4 == 0, ld % 16 == 0.  Workspace as csmae_gemm_dw_group
 * plus count * 64 * roundup(max M, 256) floats for the bias-gradient partial sums.  Fixed summation order.  timm Block backward: MAE_ViT_Baseline.py:160-188. */
int csmae_gemm_dw_group_fp8(int count, long long K, const void* const* dY, const long long* ldy, const float* const* dq_y, const void* const* X,
                            const long long* ldx, const float* const* dq_x, float* const* dW, float* const* db, const long long* M, const long long* N,
                            int slots, float* workspace, long long ws_elems, void* stream);
/* ---- fp8 MFMA path (BASELINE.json configs[4]: "fp8 MFMA GEMMs"; the same nn.Linear call sites, MAE_ViT_Baseline.py:160-188).
 * OCP fp8, per-tensor scales.  An amax is 64 partial maxima (float[64]; its value is their maximum: thousands of same-address atomics per
 * launch serialise in L2): csmae_fp8_amax folds max|x| into slots the caller zeroed; csmae_fp8_quantize writes
 * q = fp8(x * FMAX / amax) (fmt 0 = e4m3, 1 = e5m2; transpose = 1 writes dst[c][r], the mirror of a weight the dX products read) and
 * the de-quantisation factor dq = amax / FMAX; with amax_next the amax passed in is the previous step's (one pass over the tensor,
 * out-of-range values saturate) and this step's is recorded for the next.  csmae_gemm_fp8: C[M,N] = dq_a * dq_b * sum_k A8(m,k) B8(n,k) with both operands
 * K-contiguous fp8 bytes (A in a_fmt, B e4m3), fp32 accumulation (v_mfma_scale_f32_16x16x128_f8f6f4), epilogues of csmae_gemm.  With the fused fp8 copy
 * (q_out) and an epilogue without a residual, C may be NULL: the copy (and the gelu' codes) is then the product's only output — fp8 mode's steady state,
 * where the next product, the weight gradients and the bias gradients all read the fp8 bytes. */
int csmae_fp8_amax(int in_dtype, long long rows, int cols, const void* src, long long ld, float* amax, void* stream);
int csmae_fp8_quantize(int in_dtype, int fmt, int transpose, long long rows, int cols, const void* src, long long ld, void* dst,
                       long long ldd, const float* amax, float* dq, float* amax_next /* nullable: delayed scaling, += max|src| */, void* stream);
/* every fp8 weight mirror of a model in three launches (amax, W8, W8^T; blockIdx.y = weight): desc (device, 3 int64 per weight) = {offset of the
 * fp32 master in p — the same offset is used in the byte mirrors w8 ([out][in]) and w8t ([in][out]) —, out, in}; amax [count][64] zeroed by the
 * caller, dq [count] receives the de-quantisation factors (current scaling, e4m3). */
int csmae_fp8_weights(int count, const long long* desc, const float* p, void* w8, void* w8t, float* amax, float* dq, void* stream);
int csmae_gemm_fp8(int a_fmt, long long M, long long N, long long K, const void* A, long long lda, const void* B, long long ldb,
                   void* C, long long ldc, int c_dtype, const float* bias, int epilogue, void* aux, long long ldaux,
                   const void* resid, long long ldr, const float* dq_a, const float* dq_b,
                   void* q_out /* nullable: also emit C as fp8 bytes [M][ldq] in q_fmt for the GEMM that reads it next (delayed scaling) */,
                   long long ldq, int q_fmt, const float* q_amax_prev /* [64] */, float* q_amax_next /* [64] */, float* q_dq, void* stream);
/* tuning hook for tools/gemm_bench.py: force the bf16 block tile (0: 128x128, 1: 256x128, 2: 256x256, -1: heuristic) */
int csmae_gemm_force_tile(int cfg);
/* which kernel the next call with these arguments would launch (added within ABI version 7: no existing entry point changed; no launch): csmae_gemm_route for csmae_gemm — the bf16 tile
 * configuration 0..6 (0: 128x128, 2: 256x256, 4: 256x256 pipelined, 5: 192x256 pipelined, 6: 128x256 two workgroups per CU; 1 / 3 only when
 * forced) or CSMAE_GEMM_ROUTE_F32 —, csmae_gemm_ks_route for csmae_gemm_ks: CSMAE_GEMM_ROUTE_KSLAB, or the csmae_gemm route of its plain-weight
 * fallback.  Both follow csmae_gemm_force_tile and csmae_gemm_k2_mode as they stand; the answer depends on pointers only through the
 * alignment csmae_gemm_ks checks.  Negative: unsupported dtype. */
#define CSMAE_GEMM_ROUTE_F32 7
#define CSMAE_GEMM_ROUTE_KSLAB 8
int csmae_gemm_route(int dtype, int transA, int transB, long long M, long long N, long long K, long long lda, long long ldb, long long ldc,
                     int epilogue, int splitk);
int csmae_gemm_ks_route(int dtype, long long M, long long N, long long K, const void* A, long long lda, const void* Bk, long long slab_rows,
                        long long ldb_plain, const void* C, long long ldc, int epilogue);

/* ---- softmax attention of timm Block (Attention.forward: softmax(q k^T * hd^-0.5) v), qkv is [B*T, 3*H*hd]
 * in timm's (3, H, hd) column order; out [B*T, H*hd]; lse [B, H, T] (natural log). */
int csmae_attn_fwd(int dtype, long long B, int T, int H, int hd, const void* qkv, void* out, float* lse, void* stream);
int csmae_attn_bwd(int dtype, long long B, int T, int H, int hd, const void* qkv, const void* out, const void* dout,
                   const float* lse, void* dqkv, void* stream);
/* which kernel family the next csmae_attn_fwd / csmae_attn_bwd call with these arguments runs (added within ABI version 7: no existing entry point
 * changed; no launch): CSMAE_ATTN_ROUTE_RESIDENT — bf16 MFMA kernels with the whole K and V of a (sample, head) in LDS (the shapes csmae_attn_resident
 * lists) —, CSMAE_ATTN_ROUTE_STREAM — bf16 MFMA kernels that stream K / V (Q / dO) tiles, online softmax: any T <= 8192, head_dim % 8 == 0,
 * head_dim <= 128 —, CSMAE_ATTN_ROUTE_ANY — the scalar any-length kernels — or CSMAE_ATTN_ROUTE_F32 (fp32 parity mode).  Negative: unsupported dtype
 * or geometry.  Same reference expression for every route (timm Attention.forward inside Block, models_mae/MAE_ViT_Baseline.py:160-188).
 * csmae_attn_stream_mode(mode) sets the choice and returns the previous mode: 0 never stream (the routing before the streaming kernels: A/B runs),
 * 1 stream what is not resident (default), 2 stream every bf16 shape with head_dim % 8 == 0, resident ones too (tests, A/B); any other value only
 * queries.  csmae_attn_resident and the fp8-emitting csmae_attn_*_q entry points do not depend on it. */
#define CSMAE_ATTN_ROUTE_RESIDENT 0
#define CSMAE_ATTN_ROUTE_STREAM 1
#define CSMAE_ATTN_ROUTE_ANY 2
#define CSMAE_ATTN_ROUTE_F32 3
int csmae_attn_route(int dtype, int T, int hd);
int csmae_attn_stream_mode(int mode);
/* fp8 mode (BASELINE configs[4]): the same two kernels also leave their output as OCP fp8 bytes for the nn.Linear that consumes it —
 * attn.proj forward reads `out` (q_fmt 0: e4m3), attn.qkv's backward reads dqkv (q_fmt 1: e5m2) — quantised from the rounded bf16 values
 * with FMAX / max(q_amax_prev[64]) (the tensor's amax one step earlier: delayed scaling, conventions of csmae_gemm_fp8); q_amax_next[64]
 * receives partial maxima of |x|, q_dq[0] the de-quantisation factor.  bf16 shapes of the LDS-resident kernels only: csmae_attn_resident().
 * Same reference expression (timm Attention inside Block, models_mae/MAE_ViT_Baseline.py:160-188); replaces a csmae_fp8_quantize pass.
 * csmae_attn_bwd_q: dqkv may be NULL — the fp8 copy is then the only output (no reader of the bf16 gradient in fp8 mode's steady state). */
int csmae_attn_resident(int dtype, int T, int hd);
int csmae_attn_fwd_q(int dtype, long long B, int T, int H, int hd, const void* qkv, void* out, float* lse, void* q_out, int q_fmt,
                     const float* q_amax_prev, float* q_amax_next, float* q_dq, void* stream);
int csmae_attn_bwd_q(int dtype, long long B, int T, int H, int hd, const void* qkv, const void* out, const void* dout, const float* lse,
                     void* dqkv, void* q_out, int q_fmt, const float* q_amax_prev, float* q_amax_next, float* q_dq, void* stream);

/* ---- nn.LayerNorm(eps=1e-6) (MAE_ViT_Baseline.py:43-45): x [M,D] in x_dtype (the residual stream: fp32, or bf16 in throughput
 * mode); y in out_dtype (+ optional fp32 copy y32); statistics in fp32.
 * bwd: dx_out = dres_in + LN'(dy), both in x_dtype (the residual-gradient stream); dx_lp = optional low-precision copy for the next
 * GEMM (with a bf16 stream dx_out is that operand); dgamma/dbeta += via per-block partial rows in partial_ws (>= 2*D floats per
 * block; null -> atomics).  dgamma == NULL with a workspace: the partial rows (min(ceil(M/4), 1024, partial_elems / 2D) of them) are
 * left there for csmae_ln_param_reduce, which folds a whole batch of LayerNorms in one launch off the critical path.
 * q_out (nullable; fp8 mode, delayed scaling): the output that feeds the next GEMM (y / dx_out) also leaves as fp8 bytes [M][D] in q_fmt,
 * scaled with q_amax_prev (64 partial maxima), the new amax folded into q_amax_next (64 slots), the de-quantisation factor in q_dq.
 * fwd with q_out: y may be NULL — only the fp8 copy (and mean / rstd) is written (fp8 mode's steady state: every reader of y takes the fp8 bytes). */
int csmae_layernorm_fwd(int x_dtype, int out_dtype, long long M, int D, const void* x, const float* gamma, const float* beta, float eps,
                        void* y, float* y32, float* mean, float* rstd, void* q_out, int q_fmt, const float* q_amax_prev,
                        float* q_amax_next, float* q_dq, void* stream);
int csmae_layernorm_bwd(int dy_dtype, int x_dtype, int lp_dtype, long long M, int D, const void* dy, const void* x, const float* mean,
                        const float* rstd, const float* gamma, const void* dres_in, void* dx_out, void* dx_lp,
                        float* dgamma, float* dbeta, float* partial_ws, long long partial_elems, void* q_out, int q_fmt,
                        const float* q_amax_prev, float* q_amax_next, float* q_dq, void* stream);
/* LayerNorm k of the batch: partial rows at partials + k * stride (slice_elems floats each, written by csmae_layernorm_bwd with the same
 * M and D), dgamma at gbase + goff[2k], dbeta at gbase + goff[2k+1] (device array).  Fixed summation order, no atomics. */
int csmae_ln_param_reduce(int count, long long M, int D, const float* partials, long long stride, long long slice_elems,
                          float* gbase, const long long* goff, void* stream);
/* the same fold with the number of partial rows per LayerNorm given by the caller (csmae_gemm_ln_bwd leaves ceil(M / 128) of them); stride >= rows * 2 * D */
int csmae_ln_param_reduce_rows(int count, int rows, int D, const float* partials, long long stride, float* gbase, const long long* goff, void* stream);

/* ---- predictor BatchNorm1d(num_patches) + ReLU (models_mae/MLP.py:7-8): channel = token position, batch statistics
 * over (sample, feature); updates running stats (momentum, unbiased var) and num_batches_tracked in place. */
int csmae_bnrelu_fwd(int dtype, int N, int L, int Hp, const void* u, const float* gamma, const float* beta, float eps,
                     float momentum, void* r, float* mean, float* rstd, float* running_mean, float* running_var,
                     long long* num_batches_tracked, int training, void* stream);
int csmae_bnrelu_bwd(int dtype, int N, int L, int Hp, const void* u, const void* dr, const float* gamma, const float* beta,
                     const float* mean, const float* rstd, void* du, float* dgamma, float* dbeta, void* stream);

/* ---- MAE_ViT_MsLd.py:29-35,52: crop box (device int[4] i,j,h,w) + bilinear anti-aliased resize back to SxS */
int csmae_crop_resize(long long planes, int S, const float* src, float* dst, const int* box, void* stream);
/* ---- MAE_ViT_Shared.random_masking (:57-84): stable ascending argsort of noise; int64 ids_restore, f32 mask, kept ids */
int csmae_mask_sort(long long rows, int L, int keep, const float* noise, long long* ids_restore, float* mask, int* ids_keep,
                    int* ids_shuffle, void* stream);
/* ---- timm PatchEmbed on the kept patches (MAE_ViT_Baseline.py:245,251): im2col rows for the patch-embed GEMM */
int csmae_patch_gather(int dtype, long long rows, int keep, int N, int C, int S, int p, const float* img0, const float* img1,
                       const int* ids_keep, void* out, long long ld, void* stream);
/* ---- MAE_ViT_Baseline.py:248,253-256: + encoder_pos_embed, cls prepend (and its backward) */
int csmae_embed_assemble(int x_dtype, long long B2, int keep, int D, const float* tok, const float* pos, const float* cls, const int* ids_keep,
                         void* x, void* stream);
int csmae_embed_assemble_bwd(int in_dtype, int dtype, long long B2, int keep, int D, const void* dx, void* dtok, float* dcls, void* stream);
/* ---- MAE_ViT_Baseline.forward_decoder (:273-283): mask-token fill, gather(ids_restore), + decoder_pos_embed */
int csmae_unshuffle_fwd(int x_dtype, long long B2, int L, int keep, int Dd, const float* z, const float* mask_token, const float* dpos,
                        const long long* ids_restore, void* xd, void* stream);
int csmae_unshuffle_bwd(int in_dtype, int dtype, long long B2, int L, int keep, int Dd, const void* dxd, const long long* ids_restore, void* dz,
                        float* dmask_token, void* stream);
/* ---- `[:, 1:, :]` views around the predictor (MAE_ViT_MsLdCeCd.py:57-58) */
int csmae_rows_gather(int dtype, long long rows, int D, const float* src, long long group, long long gstride, long long off,
                      void* dst, void* stream);
int csmae_rows_scatter_add(int dtype, long long rows, int D, const void* src, float scale, long long group, long long gstride,
                           long long off, float* dst, void* stream);
/* two sources into two row views of the same buffer in one pass: dst[view(r) + off_a] += scale_a a[r], dst[view(r) + off_b] += scale_b b[r]
 * (the cross-decoder loss' gradient w.r.t. its target — the original's decoder embedding — and the predictor's input gradient — the
 * crop's —, MAE_ViT_MsLdCeCd.py:56-59: `loss_cd(x_embed_orig[:, 1:], predictor(x_embed_crop[:, 1:]))`, target not detached). */
int csmae_rows_scatter_add2(int dtype, long long rows, int D, const void* a, float scale_a, long long off_a, const void* b, float scale_b, long long off_b,
                            long long group, long long gstride, float* dst, void* stream);
/* The cross-decoder head's backward chain run AHEAD of the upstream gradient (ABI version 7): pair loss -> predictor Linear -> BatchNorm / ReLU -> Linear
 * depends on d(loss) only through a scalar factor, so csmae_hip runs it with unit gradient at the end of the forward pass (it is the longest chain of the
 * forward / backward junction); when the real factor g (device scalar) arrives, this call adds g x (tmp_dgamma, tmp_dbeta) — BatchNorm's parameter
 * gradients of the unit run — into dgamma / dbeta and scales the chain's three bf16 gradient tensors (n0 / n1 / n2 elements) by g in place: nothing to
 * scale when g == 1.  MAE_ViT_MsLdCeCd.py:56-59 backward. */
int csmae_spec_fixup(const float* g, void* b0, long long n0, void* b1, long long n1, void* b2, long long n2, const float* tmp_dgamma, const float* tmp_dbeta,
                     float* dgamma, float* dbeta, int L, void* stream);
/* MAE_ViT_Shared.py:77 (`torch.gather(x, dim=1, index=ids_keep.unsqueeze(-1).repeat(1, 1, D))` of the stand-alone random_masking):
 * out[n, k, :] = x[n, ids[n * ids_ld + k], :], x [N, L, D] fp32, ids int32 (csmae_mask_sort's ids_keep), out [N, keep, D] fp32. */
int csmae_rows_gather_idx(long long N, int L, int keep, int D, const float* x, const int* ids, long long ids_ld, float* out, void* stream);

/* ---- MAE_ViT_Shared.forward_loss (:269-290) with process_target/patchify fused (:24-39,97-111).
 * pred is [B2*(L+1), ldp] (row 0 of every sample = cls, ignored) in `pred_dtype` (fp32, or the bf16 the throughput path's decoder_pred
 * product writes — what autocast hands the reference's loss); rowloss [B2*L].  fwd: `mask` (nullable, [B2*L]) lets the kernel skip the
 * patches the loss does not weigh (:113-120): their rowloss is 0. */
int csmae_target_minmax(int norm_pix, long long B2, int N, int C, int S, int p, const float* img0, const float* img1,
                        float* scratch, float* out, void* stream);
int csmae_recon_loss_fwd(int kind, int norm_pix, int pred_dtype, long long B2, int N, int C, int S, int p, const float* img0, const float* img1,
                         const void* pred, long long ldp, const float* minmax, const float* mask, float* rowloss, void* stream);
int csmae_recon_loss_bwd(int kind, int norm_pix, int out_dtype, int pred_dtype, long long B2, int N, int C, int S, int p, const float* img0,
                         const float* img1, const void* pred, long long ldp, const float* minmax, const float* mask,
                         const float* losses, const float* gout, float vscale, const float* extra, void* dpred, long long ldd,
                         void* stream);
/* ---- the ssim family of reconstruction losses: MAE_ViT_Shared.forward_loss_{ssim,ms_ssim} (:165-247) around
 * pytorch-msssim 0.2.1 ssim / ms_ssim (:204,:247).  levels = 1 (ssim, nonnegative) or 5 (ms_ssim).  `ws` holds the image planes,
 * partial sums and statistics between the calls (csmae_ssim_workspace_floats floats, caller-allocated, untouched between fwd and bwd).
 * fwd: terms[v] = 1 - score of view v.   apply (after csmae_loss_finalize): losses[1+v] (+)= weight * terms[v], total fixed up
 * (`pure` = no per-patch term, the plain ssim / ms_ssim kinds; otherwise the 0.1-weighted mse_* kinds :249-267).
 * flags serve util/metrics.py (ssim / ms_ssim of two image batches in [0, 1], :4-10,:41-46): 1 = no min-max scaling, 2 = no relu.
 * bwd: extra[B2*L][P] (fp32) = gout * scale * d terms / d pred, handed to csmae_recon_loss_bwd (kind 5 = no per-patch term). */
int csmae_ssim_workspace_floats(long long B2, int C, int S, int p, int levels, long long* floats /* host pointer, out */);
int csmae_ssim_fwd(int levels, int flags /* 1: operands as they are (no scale_01) | 2: signed single-scale score */, int norm_pix,
                   long long B2, int N, int C, int S, int p, const float* img0, const float* img1, const float* pred, long long ldp,
                   const float* mask, float* ws, float* terms, void* stream);
int csmae_ssim_apply(int pure, int views, float weight, float recon_scale, const float* terms, float* losses, void* stream);
int csmae_ssim_bwd(int levels, long long B2, int N, int C, int S, int p, const float* pred, long long ldp, const float* mask,
                   const float* gout, float scale, float* ws, float* extra, void* stream);
/* ---- un-masked `.mean()` losses: cross-decoder (MAE_ViT_MsLdCeCd.py:56-59, target NOT detached) and latent (MsLdLe.py:44) */
int csmae_pair_loss_fwd(int kind, long long rows, int D, const float* a, long long a_group, long long a_gstride, long long a_off,
                        const float* t, long long t_group, long long t_gstride, long long t_off, float* partial, void* stream);
int csmae_pair_loss_bwd(int kind, int lp_dtype, long long rows, int D, const float* a, long long a_group, long long a_gstride,
                        long long a_off, const float* t, long long t_group, long long t_gstride, long long t_off,
                        const float* gout, float coef, void* da_lp, float* da_acc, float* dt_acc, void* stream);
/* ---- util/contrast_loss.NTXentLoss(bs, 0.5, cos_sim=True) on mean-pooled latents (MAE_ViT_MsLdCeCd.py:61-69) */
int csmae_ntxent_fwd(int N, int Te, int keep, int D, const float* latent, float tau, float eps, float* z, float* inv_norm,
                     float* E, float* neg, float* rowloss, void* stream);
int csmae_ntxent_bwd(int N, int D, const float* z, const float* inv_norm, const float* E, const float* neg, float tau, float eps,
                     const float* gout, float* dpool, void* stream);
int csmae_latent_grad_finish(int lp_dtype, long long B2, int Te, int D, float* dlat, const float* dpool, float inv_keep,
                             void* dlat_lp, void* stream);
/* ---- scalar assembly: losses[0]=total [1]=recon orig [2]=recon crop [3]=cross-decoder [4]=contrastive [5]=latent
 *      [6],[7]=sum(mask) per view (MAE_ViT_MsLd.py:64-66, MAE_ViT_MsLdCeCd.py:72) */
int csmae_loss_finalize(long long per_view, int views, const float* rowloss, const float* mask, float recon_scale,
                        const float* cd_partial, float cd_scale, const float* e_partial, float e_scale,
                        const float* ce_rowloss, int ce_rows, float* losses, void* stream);

/* ---- input step before the path (util/datasets.py:120-136 training transform): decoded uint8 HWC images ->
 * ToTensor, Normalize(mean, std), horizontal / vertical flip, RandomResizedCrop(S, bicubic, antialias) in one kernel.
 * src [N, Hmax, Wmax, C] u8 (image n in the top-left H x W corner), meta [N, 8] int32 = {H, W, i, j, h, w, hflip, vflip}
 * (box in the coordinates of the flipped image; drawn on the host in torchvision's RNG order), dst [N, C, S, S] fp32. */
int csmae_augment_u8(long long N, int C, int Hmax, int Wmax, int S, const unsigned char* src, const int* meta, const float* mean,
                     const float* inv_std, float* dst, void* stream);
/* the eval transform (util/datasets.py:140-158): ToTensor, Normalize, Resize(int(S / crop_pct), bicubic, antialias), CenterCrop(S).
 * Same src / dst layout; meta [N, 8] int32 = {H, W, Hr, Wr, top, left, 0, 0}: output pixel (oy, ox) is pixel (oy + top, ox + left) of the
 * H x W -> Hr x Wr resize.  The host (util/gpu_input.py eval_transform_params) computes meta and refuses sizes the kernel cannot hold. */
int csmae_eval_u8(long long N, int C, int Hmax, int Wmax, int S, const unsigned char* src, const int* meta, const float* mean,
                  const float* inv_std, float* dst, void* stream);
/* The same two transforms for multispectral tiles (util/datasets.py:489-564, Dataset_eurosat; added within ABI version 7, csrc/multispectral.hip):
 * src [N, Hmax, Wmax, Cin] uint16 in raw units (no / 255), meta as for the u8 pair, dst [N, Cout, S, S] fp32, 1 <= Cout <= Cin <= 13 and
 * Wmax * Cin <= 12288.  band [Cout] int32 is a HOST array, read and checked before the launch: output channel k is source band band[k] & 0xFF;
 * with bit 8 set the band is masked (every source value counts as mean[k], so the channel is exactly 0).  A source band that no entry names is
 * dropped and never read.  mean, inv_std [Cout] fp32 on the device, in raw units, already gathered to the output channels. */
int csmae_augment_u16(long long N, int Cin, int Cout, int Hmax, int Wmax, int S, const unsigned short* src, const int* meta,
                      const int* band, const float* mean, const float* inv_std, float* dst, void* stream);
int csmae_eval_u16(long long N, int Cin, int Cout, int Hmax, int Wmax, int S, const unsigned short* src, const int* meta,
                   const int* band, const float* mean, const float* inv_std, float* dst, void* stream);

/* ---- optimizer side (main_pretrain.py:426-427 torch.optim.AdamW; util/misc.py:314 backward products) */
/* gate (nullable device scalar): the update is skipped as a whole when it is not finite — engine_pretrain.py:56-58 raises on a
 * non-finite loss BEFORE backward / step; here the loss stays on the device and the kernel keeps the poisoned step out of the weights. */
/* tile_ks / p_ks (nullable, ABI 6): the launch also writes the K-slab mirrors (csmae_gemm_ks) of the weights it steps — tile_ks[tile] =
 * {flat offset of the tile's weight, N, K} (device int64 [ntiles][3]; K = 0: none) — so that no csmae_weights_kslab launch is needed per step. */
int csmae_adamw(long long ntiles, const long long* tile_off, const int* tile_cnt, const float* tile_wd, float* p, const float* g,
                float* m, float* v, float lr, float beta1, float beta2, float eps, float bias_correction1, float bias_correction2,
                void* p_lp, const float* gate, const long long* tile_ks, void* p_ks, void* stream);
/* The same step for the block Linear weights of an fp8-mode model (ABI version 7), writing their fp8 mirrors on the way: W8 [out][in] (e4m3) for the forward
 * products, W8^T [in][out] for dX — instead of csmae_fp8_weights' three launches per step.  tile8: device int64 [ntiles][6] = {flat offset of the weight,
 * N = out, K = in (multiples of 64), n0, k0 (the workgroup's 64 x 64 sub-block), weight index}.  Delayed scaling: scale 448 / amax_prev[w] (64 partial
 * maxima per weight, one step old), the new maximum into amax_next[w] (zeroed by the caller), dq[w] = amax_prev[w] / 448.  One weight-decay value per launch. */
int csmae_adamw_fp8(long long ntiles, const long long* tile8, float weight_decay, float* p, const float* g, float* m, float* v, float lr, float beta1,
                    float beta2, float eps, float bias_correction1, float bias_correction2, void* p_lp, const float* gate, void* w8, void* w8t,
                    const float* amax_prev, float* amax_next, float* dq, void* stream);
int csmae_gate_accumulate(const float* loss, float* slot, int accumulate, void* stream);
/* util/misc.py:310-318 (`torch.nn.utils.clip_grad_norm_(parameters, clip_grad)`) / :338-355 (`get_grad_norm_`) on the flat gradient
 * buffer: out[0] = total 2-norm, out[1] = min(1, max_norm / (norm + 1e-6)); g *= out[1] in place when max_norm > 0 (<= 0: norm only).
 * scratch: >= 1024 floats.  No host synchronisation. */
int csmae_clip_grad_norm(long long n, float* g, float max_norm, float* scratch, float* out, void* stream);
int csmae_cast_f32_to_bf16(long long n, const float* src, void* dst, void* stream);
int csmae_cast_bf16_to_f32(long long n, const void* src, float* dst, void* stream);
int csmae_colsum(int dtype, long long M, int N, const void* x, long long ld, float* out, void* stream);

/* ---- linear probing of the frozen encoder (main_linprobe.py:515-525; added within ABI version 7, csrc/classify.hip).  All fp32 except the
 * token stream x of the pooling kernel. */
/* models_vit.py:53-58 behind the last block: global_pool = 1: mean over tokens 1 .. T-1, then LayerNorm (fc_norm); 0: LayerNorm of token 0 (norm).
 * x [N, T, D] fp32 or bf16 (16-byte aligned, D % 4 == 0, D <= 4096), feat [N, D] fp32.  global_pool with T = 1 is refused. */
int csmae_probe_pool_fwd(int dtype, int global_pool, long long N, int T, int D, const void* x, const float* gamma, const float* beta, float eps,
                         float* feat, void* stream);
/* BatchNorm1d(D, affine=False) over the batch axis of feat [N, D].  training: biased batch variance normalises, running_mean / running_var move
 * with `momentum` (unbiased variance), num_batches_tracked (nullable) += 1; N = 1 is refused.  Otherwise the running statistics normalise. */
int csmae_bn1d_fwd(long long N, int D, const float* feat, float eps, float momentum, float* fbn, float* running_mean, float* running_var,
                   long long* num_batches_tracked, int training, void* stream);
/* logits [N, K] = x [N, D] w[K, D]^T + b (b nullable); any K, any D */
int csmae_head_linear_fwd(long long N, int D, int K, const float* x, const float* w, const float* b, float* logits, void* stream);
/* dw [K, D] (+)= gscale dlogits^T x, db [K] (+)= gscale sum_n dlogits (db nullable; gscale: nullable device scalar, 1 when absent) */
int csmae_head_linear_bwd(long long N, int D, int K, const float* dlogits, const float* x, const float* gscale, float* dw, float* db, int accumulate,
                          void* stream);
/* mean cross-entropy of logits [N, K] against labels [N] (int64) -> loss[0]; dlogits (nullable) = gout (softmax - onehot) / N (gout: nullable
 * device scalar); counts (nullable) [2] (+)= rows whose label is in the top 1 / top min(5, K) (fewer than k logits strictly greater than the
 * label's).  A label outside [0, K) gives a NaN loss and gradient row and no hit.  scratch: 3 N floats. */
int csmae_softmax_ce(long long N, int K, const float* logits, const long long* labels, const float* gout, float* scratch, float* loss, float* dlogits,
                     float* counts, int accumulate_counts, void* stream);
/* LARS (util/lars.py:27-57) over ntensors tensors: table (device int64 [ntensors][5]) = {p, g, mu addresses, numel, ndim > 1}.  Matrices:
 * dp = q (g + wd p), q = trust |p| / |dp| (1 when either norm is 0); vectors: dp = g.  mu = momentum mu + dp, p -= lr mu.  norms: ntensors x 128
 * floats of scratch.  gate: nullable device scalar, a non-finite value skips the whole update.  Two launches, no host synchronisation. */
int csmae_lars_step(int ntensors, const long long* table, float lr, float weight_decay, float momentum, float trust, float* norms, const float* gate,
                    void* stream);

/* ---- end-to-end fine-tuning (main_finetune.py, engine_finetune.py; added within ABI version 7, csrc/classify.hip).  No atomics: two runs give the
 * same bits. */
/* Reverse of csmae_probe_pool_fwd: recomputes the pooled row and its LayerNorm statistics from x [N, T, D] (fp32 or bf16), applies the LayerNorm
 * backward to dfeat [N, D] and writes the WHOLE gradient dres [N, T, D] (the dtype of x): global_pool = 1: rows 1 .. T-1 get dpooled / (T - 1), row
 * 0 zero; 0: row 0 gets the gradient, the others zero.  dgamma / dbeta [D] (+)= the sum over N in sample order (partial: 2 N D floats of scratch).
 * x, dres 16-byte aligned, D % 4 == 0, D <= 4096; global_pool with T = 1 is refused. */
int csmae_probe_pool_bwd(int dtype, int global_pool, long long N, int T, int D, const void* x, const float* dfeat, const float* gamma, float eps,
                         void* dres, float* partial, float* dgamma, float* dbeta, int accumulate, void* stream);
/* dx [N, D] = gscale dlogits [N, K] w [K, D] (gscale: nullable device scalar, 1 when absent) */
int csmae_head_linear_dx(long long N, int D, int K, const float* dlogits, const float* w, const float* gscale, float* dx, void* stream);
/* soft-target cross-entropy (timm SoftTargetCrossEntropy): loss[0] = mean_n sum_k -target[n, k] log_softmax(logits)[n, k]; dlogits (nullable) =
 * gout (softmax sum_k target - target) / N (gout: nullable device scalar).  target: dense fp32 [N, K].  scratch: N floats. */
int csmae_soft_ce(long long N, int K, const float* logits, const float* target, const float* gout, float* scratch, float* loss, float* dlogits,
                  void* stream);
/* dense targets [N, K] from labels [N] (int64), timm mixup_target: lam onehot(y[n], on, off) + (1 - lam) onehot(y[N-1-n], on, off) with
 * off = smoothing / K, on = 1 - smoothing + off; lam = 1 is plain label smoothing.  A label outside [0, K) indexes nothing. */
int csmae_mixup_target(long long N, int K, const long long* labels, float lam, float smoothing, float* target, void* stream);
/* batch-mode mixing of x [N, C, H, W] fp32 with the flipped batch, out of place (out != x), N even.  cutmix = 0: out[n] = lam x[n] + (1 - lam)
 * x[N-1-n]; 1: out[n] = x[n] with rows [yl, yh) x columns [xl, xh) copied from x[N-1-n] (lam unused). */
int csmae_mixup_cutmix(int cutmix, long long N, int C, int H, int W, const float* x, float* out, float lam, int yl, int yh, int xl, int xh,
                       void* stream);
/* dpos [T, D] (+)= sum_n dres[n] for dres [N, T, D] fp32 or bf16, fp32 accumulation in sample order */
int csmae_pos_embed_grad(int dtype, long long N, int T, int D, const void* dres, float* dpos, int accumulate, void* stream);

/* ---- k-NN evaluation of the frozen encoder (main_knn.py, csmae_hip/knn.py; added within ABI version 7, csrc/knn.hip).  The similarities themselves
 * come from csmae_gemm; these are the steps around it.  One wave per row; no atomics: two runs give the same bits. */
/* dst [rows, D] (dense; out_dtype fp32 or bf16) = src[r] / max(||src[r]||_2, eps), src fp32 with leading dimension ld >= D, the squares summed in
 * fp32.  Any D. */
int csmae_l2_normalize(int in_dtype, int out_dtype, long long rows, int D, const void* src, long long ld, float eps, void* dst, void* stream);
/* Merge one similarity tile into the running best-k lists.  sim: fp32 [Q, Bc] with leading dimension ld >= Bc (columns Bc .. ld-1 are never read),
 * the similarities of Q queries to bank rows base .. base+Bc-1.  val [Q, k] fp32 / idx [Q, k] int32: each query's list, read and rewritten, ordered
 * by (similarity descending, bank index ascending); unused slots are (-inf, -1), and a search starts from lists filled with exactly that.  Once
 * tiles covering the bank have been merged — in any chunking and any order — the lists equal a stable descending sort of the whole similarity row cut
 * at k, bit for bit.  1 <= k <= 64 (one lane of a wave per entry): anything else is refused before a launch.  Rows that are 16-byte aligned (sim
 * aligned, ld % 4 == 0) are read as float4. */
int csmae_knn_select(long long Q, int Bc, int k, const float* sim, long long ld, long long base, float* val, int* idx, void* stream);
/* The weighted vote of DINO's knn_classifier over lists as csmae_knn_select leaves them: votes [Q, K] (nullable) [q, c] = sum over j with idx[q, j] >= 0
 * and bank_labels[idx[q, j]] == c of exp(val[q, j] * inv_T), added in list order (bank_labels int64; one outside [0, K) votes for nothing).
 * top5 [Q, 5] int32 = the five classes with the largest votes, descending, ties to the lower class id, -1 behind the K-th when K < 5.  With
 * query_labels (int64, nullable) counts [2] (+)= the queries whose label is top5[0] / among top5, as csmae_softmax_ce's counters (accumulate_counts);
 * without them counts is left alone.  1 <= k <= 64, 1 <= K <= 2048. */
int csmae_knn_vote(long long Q, int k, int K, const float* val, const int* idx, const long long* bank_labels, float inv_T, float* votes, int* top5,
                   float* counts, const long long* query_labels, int accumulate_counts, void* stream);

/* ---- per-image reconstruction scores of a batch (util/metrics.py batch_metrics, util/viz.py run_eval; added within ABI version 7,
 * csrc/recon_eval.hip).  With X = img * std + mean and Y = the un-patchified pred * std + mean (mean, std: [C] fp32 on the device):
 *   out[n] = { sum (X - Y)^2, sum |X - Y|, ssim(X, Y), 0 }   (fp32 [N][4]; the sums run over all C S S elements of image n)
 * ssim is pytorch-msssim 0.2.1's (11-tap gaussian, sigma 1.5, valid windows, data_range 1, signed: no relu), the mean over the C planes.
 * img: fp32 [N, C, S, S].  pred (pred_dtype fp32 or bf16): patch row l = (y / p) (S / p) + x / p of image n starts at pred + n img_stride + l ldp
 * and holds pixel (c, y, x) at element ((y % p) p + x % p) C + c; ldp >= p p C, elements behind a row's p p C are never read.  A cls row in
 * front of each image's rows is skipped by the caller: pass pred + ldp and img_stride = (L + 1) ldp.  part: csmae_recon_eval_workspace_floats
 * floats.  No plane is written to memory; two launches, no atomics; an image's four floats depend on that image alone (not on N, not on n).
 * Refused before any launch: S < 11, S % p != 0, C < 1, a null pointer, a pred_dtype other than fp32 / bf16. */
int csmae_recon_eval_workspace_floats(long long N, int C, int S, long long* floats /* host pointer, out */);
int csmae_recon_eval(int pred_dtype, long long N, int C, int S, int p, const float* img, const void* pred, long long ldp, long long img_stride,
                     const float* mean, const float* std, float* part, float* out, void* stream);

/* ---- reconstruction contact sheets of a batch (util/viz.py reconstruction_panels, plot_reconstruction, run_eval; added within ABI version 7,
 * csrc/recon_panel.hip).  out: uint8 [N][S][W][3], W = n_panels S + (n_panels - 1) gap, dense: per image one RGB row of n_panels panels with gap
 * white (255) pixels between neighbours.  img, pred (pred_dtype, ldp, img_stride), mean, std: as csmae_recon_eval takes them.  mask: fp32 [N][L],
 * L = (S / p)^2, 1 = patch removed, 0 = kept.  With X = img * std + mean, Y = the un-patchified pred * std + mean and m = mask of the pixel's patch,
 * panel k shows, by its code panel<k> (panel<k> with k >= n_panels is ignored):
 *   0 x: X    1 xm: X (1 - m)    2 y: Y    3 ym: Y m    4 xm_ym: X (1 - m) + Y m
 * of the channels band_r, band_g, band_b (each in [0, C); C = 1: 0, 0, 0), every value v as the byte (int) min(max(255 v, 0), 255), truncating;
 * a NaN gives 0, +inf 255, -inf 0, and an operand a panel does not show is not read.  One launch, no atomics, no workspace; every byte of out is
 * written exactly once (out need not be cleared, and needs no alignment); an image's bytes depend on that image alone (not on N, not on n).
 * Refused before any launch: a null pointer, N <= 0, S % p != 0, ldp / img_stride too small, a pred_dtype other than fp32 / bf16, a band outside
 * [0, C), n_panels outside [1, 5], a code outside [0, 4], gap < 0, a sheet of 2^31 bytes or more, more workgroups than the grid holds. */
int csmae_recon_panel(int pred_dtype, long long N, int C, int S, int p, const float* img, const void* pred, long long ldp, long long img_stride,
                      const float* mask, const float* mean, const float* std, int band_r, int band_g, int band_b, int panel0, int panel1, int panel2,
                      int panel3, int panel4, int n_panels, int gap, unsigned char* out, void* stream);

/* ---- linear segmentation probe of the frozen encoder (main_segprobe.py, models_seg.py; added within ABI version 7, csrc/segment.hip).  The head itself
 * is csmae_bn1d_fwd + csmae_head_linear_fwd / _bwd over the N L patch rows; these are the steps around it.  No floating-point atomics: two runs give
 * the same loss and gradient bits. */
/* The model's final LayerNorm on every PATCH token of the residual stream x [N, T = L + 1, D] (fp32 or bf16): the cls row of each image is dropped,
 * out [N L, D] fp32, statistics in fp32 (mean, then centred squares).  One wave per token.  No backward: the trunk and its norm are frozen in a probe. */
int csmae_seg_token_norm(int dtype, long long N, int T, int D, const void* x, const float* gamma, const float* beta, float eps, float* out,
                         void* stream);
/* Mean cross-entropy of bilinearly upsampled patch logits against per-pixel labels.  pl [N, G, G, K] fp32, labels [N, S, S] uint8 with S = G p; a
 * label of CSMAE_SEG_IGNORE takes no part.  Interpolation rule: torch.nn.functional.interpolate(mode="bilinear", align_corners=False) — an output
 * position i of an axis reads the source coordinate max((i + 0.5) / p - 0.5, 0), its integer part and the next cell clamped to G - 1, weighted by the
 * fraction; the upsampled logits never reach memory.  Per valid pixel the stable log-softmax loss (maximum subtracted);
 *   loss[0] = sum over valid pixels / count[0],  count[0] = the number of valid pixels.
 * Empty-batch convention: with no valid pixel loss[0] = 0 and csmae_seg_ce_bwd writes zeros (torch's cross_entropy gives NaN there).
 * conf (nullable) [K, K] int64, rows = true class, columns = argmax class (the lowest index wins ties), is ACCUMULATED into with integer atomics:
 * the caller zeroes it, an evaluation sweep sums over its batches.  pred (nullable) [N, S, S] uint8 receives the argmax class of EVERY pixel, ignored
 * ones too; labels may be NULL when pred is given (every pixel then counts as ignored).  Labels are the caller's contract: a value in [K, 255) is not
 * detected — it names no class (its pixel contributes its log-sum-exp to the loss, its softmax to the gradient, nothing to conf); nothing is read
 * or written out of bounds.  scratch: 2048 floats (per-workgroup partials, folded in a fixed order by a second launch).
 * Refused before any launch: K outside [2, 64], p not in {4, 8, 14, 16}, G outside [1, 4096], S != G p, N S S >= 2^31, a null pointer. */
#define CSMAE_SEG_IGNORE 255
int csmae_seg_ce(long long N, int G, int p, int K, int S, const float* pl, const unsigned char* labels, float* scratch, float* loss, long long* count,
                 long long* conf, unsigned char* pred, void* stream);
/* dpl [N, G, G, K] = gscale / count[0] * sum over pixels of w(pixel, cell) (softmax - onehot), the gradient of loss[0] (gscale: nullable device scalar,
 * 1 when absent; count: the device scalar csmae_seg_ce wrote — no host synchronisation).  A gather: each cell walks the at most 2 p x 2 p pixels
 * that read it and recomputes their softmax from pl, so every element is written exactly once, in a fixed summation order: dpl need not be cleared. */
int csmae_seg_ce_bwd(long long N, int G, int p, int K, int S, const float* pl, const unsigned char* labels, const long long* count, const float* gscale,
                     float* dpl, void* stream);
/* Overlay sheets, the argmax map and per-image counts of a batch (util/seg_viz.py segmentation_panels, main_segprobe.py --panel_dir / --pred_dir /
 * --per_image; added within ABI version 7, csrc/seg_panel.hip), from the operands csmae_seg_ce scores: the same upsampling and tie rule, the upsampled
 * logits never reach memory.  img: fp32 [N, C, S, S], normalised; mean, std: fp32 [C]; band_r, band_g, band_b: the channels shown as red, green, blue;
 * pl: fp32 [N, G, G, K], S = G p; labels (nullable): uint8 [N, S, S], CSMAE_SEG_IGNORE = ignored; palette: uint8 [K, 3] on the device; ignore_r,
 * ignore_g, ignore_b: the colour of an ignored pixel, bytes; a8: the overlay's alpha in 256ths, [0, 256].
 *   out   uint8 [N][S][W][3], W = n_panes S + (n_panes - 1) gap, dense, gap bytes 255 (csmae_recon_panel's layout); needs no alignment
 *   pred  (nullable) uint8 [N][S][S]: the argmax class of every pixel, the lowest index winning ties
 *   stats (nullable, needs labels) int32 [N][K][3]: per image and class (intersection, label area, prediction area) over the pixels whose label
 *         is < K; OVERWRITTEN (cleared on the stream, then added to with integer atomics), so the sum over n is the diagonal, the row sums and the
 *         column sums of csmae_seg_ce's conf.
 * With b = (int) min(max(255 (img std + mean), 0), 255) (csmae_recon_panel's byte), arg the argmax class and
 * blend(b, c) = (b (256 - a8) + c a8 + 128) >> 8, pane k shows by its code pane<k> (pane<k> with k >= n_panes is ignored), at a valid pixel
 * (label < K) | at an ignored one (label CSMAE_SEG_IGNORE, or a stray label in [K, 255)):
 *   0 image: b | b                              1 gt: palette[label] | ignore_rgb               2 pred: palette[arg] | the same
 *   3 gt_over: blend(b, palette[label]) | blend(b, ignore_rgb)                                   4 pred_over: blend(b, palette[arg]) | the same
 *   5 errors: blend(b, (255, 0, 0)) where arg != label, b where it is right | blend(b, ignore_rgb)
 * (The name has no underscore after "seg": the csmae_seg_* family is the probe's three training entry points above, and stays those three.)
 * One kernel launch; every byte of out and pred is written exactly once; an image's bytes and counts depend on that image alone.
 * Refused before anything is launched: a null img, mean, std, pl, palette or out; N <= 0; K outside [2, 64]; p not in {4, 8, 14, 16}; G outside
 * [1, 4096]; S != G p; n_panes outside [1, 6]; a code outside [0, 5]; a pane 1, 3 or 5, or stats, with labels null; a band outside [0, C); gap < 0;
 * a8 outside [0, 256]; an ignore colour outside [0, 255]; N S W 3 >= 2^31. */
int csmae_segpanel(long long N, int C, int S, int G, int p, int K, const float* img, const float* mean, const float* std, int band_r, int band_g,
                    int band_b, const float* pl, const unsigned char* labels, const unsigned char* palette, int ignore_r, int ignore_g, int ignore_b,
                    int a8, int pane0, int pane1, int pane2, int pane3, int pane4, int pane5, int n_panes, int gap, unsigned char* out,
                    unsigned char* pred, int* stats, void* stream);


/* ---- a stream confined to a subset of the compute units (ABI version 5).  The reference overlaps DDP's bucket all-reduces and autograd's
 * weight-gradient work with the main chain on CUDA streams that share every SM (main_pretrain.py:417-421); on MI355X a GEMM workgroup owns a
 * whole CU (160 KiB of LDS, 512 threads), so two streams time-slice CUs unless each is given its own.  `mask`: `words` x 32 bits; on this
 * 8-XCD part bit i is CU (i / 8) of XCD (i % 8) (the driver deals the bits round-robin over XCDs, then over shader engines), so the
 * first 8 n bits are n CUs of every XCD.  `*out` receives a hipStream_t (wrap it with torch.cuda.ExternalStream); destroy it with
 * csmae_stream_destroy once no work is pending on it. */
int csmae_stream_create_cu_mask(int words, const unsigned* mask, void** out);
int csmae_stream_destroy(void* stream);

#ifdef __cplusplus
}
#endif
#endif
