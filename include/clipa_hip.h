/* clipa_hip.h - C ABI of libclipa_hip.so, the MI355X (gfx950) compute engine behind the open_clip
 * model/loss API of UCSC-VLAA/CLIPA (clipa_torch).
 *
 * The reference has no FFI: its hot path is torch ops called from open_clip/{transformer,model,loss}.py.
 * Each entry point below replaces the torch op(s) at the cited reference lines (paths relative to
 * /root/reference/clipa_torch).  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch-allocated); no hidden
 *     allocations, no implicit synchronisation; `stream` is a hipStream_t;
 *   - "bf16" buffers are raw uint16 bfloat16; matrices are row-major with element strides `ld*`;
 *   - return 0 on success, negative on error (never throws); clipa_last_error() gives the message;
 *   - re-entrant: may be called from PyTorch's autograd worker thread.
 */
#ifndef CLIPA_HIP_H
#define CLIPA_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* epilogues of clipa_gemm_nt */
#define CLIPA_EPI_NONE 0 /* C = bf16(alpha*acc + bias)                                        */
#define CLIPA_EPI_ACT 1  /* C = act(v), optional C2 = v (pre-activation, for the backward)    */
#define CLIPA_EPI_ADD 2  /* C = v + aux            (residual add, transformer.py:248-249)     */
#define CLIPA_EPI_DACT 3 /* C = v * act'(aux)      (activation backward)                      */
/* MI355X engine extensions (no reference counterpart): the pre-activation kept as OCP e4m3 bytes (saturating, no scale) - half
 * the HBM of the bf16 copy.  Whole-tile shapes only (M, N multiples of 256, K multiple of 128, K >= 256): other shapes return
 * CLIPA_ERR_ARG and the caller composes CLIPA_EPI_ACT + clipa_cast_bf16_to_e4m3 / clipa_cast_e4m3_to_bf16 + CLIPA_EPI_DACT. */
#define CLIPA_EPI_ACT_PRE8 4 /* C = act(v), C2 = e4m3(v): uint8 [M, ldc]                      */
#define CLIPA_EPI_DACT8 5    /* C = v * act'(aux), aux = e4m3 bytes, uint8 [M, ldaux]; optional C2 = act(aux), bf16 [M, ldc]:
                              * what clipa_activation_fwd_e4m3 writes for the same bytes (the c_proj weight gradient's operand) */
/* activations: nn.GELU(approximate='none'|'tanh') (model.py:128-129), QuickGELU (transformer.py:37-40) */
#define CLIPA_ACT_GELU_ERF 0
#define CLIPA_ACT_GELU_TANH 1
#define CLIPA_ACT_QUICK_GELU 2
/* input dtypes of clipa_patchify */
#define CLIPA_DT_U8 0
#define CLIPA_DT_BF16 1
#define CLIPA_DT_F32 2
/* pooling modes (transformer.py:472-478, model.py:254-260) */
#define CLIPA_POOL_FIRST 0      /* x[:,0]  (cls token / big_vision_tok)          */
#define CLIPA_POOL_LAST 1       /* x[:,-1] (big_vision_last)                      */
#define CLIPA_POOL_INDEX 2      /* x[b, idx[b]] (EOT row, text.argmax(-1))        */
#define CLIPA_POOL_MEAN_ALL 3   /* x.mean(1) incl. cls (open_clip GAP)            */
#define CLIPA_POOL_MEAN_PATCH 4 /* x[:,1:].mean(1) (big_vision_gap)               */

const char* clipa_last_error(void);
int clipa_version(void);

/* C[M,N] = epi(alpha * A[M,K] . B[N,K]^T + bias[N]); A,B bf16; C bf16 (or f32 when out_f32, epi NONE).
 * Replaces nn.Linear / packed in-proj / out-proj / conv1-as-GEMM / `@ proj` forward and, with B = W^T,
 * their input gradients: transformer.py:209,217-219,234,371,491,528-529; model.py:254; loss.py:135-142.
 * K % 8 == 0; N, lda, ldb, ldc, ldaux % 8 == 0. */
int clipa_gemm_nt(const void* A, const void* B, void* C, void* C2, const float* bias, const void* aux,
                  int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldaux,
                  float alpha, int epi, int act, int out_f32, void* stream);

/* e4m3 pre-activations ("light8" keep tier): bf16 -> saturating OCP e4m3 bytes and back (exact), and act(e4m3 x) -> bf16
 * (the re-materialisation of the MLP activation in backward: transformer.py:217-219 `gelu`). */
int clipa_cast_bf16_to_e4m3(const void* in, void* out, int64_t n, void* stream);
int clipa_cast_e4m3_to_bf16(const void* in, void* out, int64_t n, void* stream);
int clipa_activation_fwd_e4m3(const void* x8, void* out, int64_t n, int act, void* stream);

/* out[R,C] = sum_m P[m,R] * Q[m,C]  (weight gradients dW = dY^T . X of the same layers; also the
 * gathered-feature gradients of loss.py:135-139).  out is f32 or bf16. workspace: split-M partial slabs. */
int64_t clipa_gemm_tn_workspace(int64_t M, int64_t R, int64_t C, int64_t* nslices);
/* colsum_out (optional, f32 [R]): column sums of P = the bias gradient of the same layer, fused into the pass. */
int clipa_gemm_tn(const void* P, const void* Q, void* out, float* colsum_out, int64_t M, int64_t R, int64_t C,
                  int64_t ldp, int64_t ldq, int out_bf16, void* workspace, int64_t workspace_bytes, void* stream);

/* fp8 path (BASELINE.json configs[3]: "fp8 MFMA weights/activations"; the reference's precision menu,
 * training/params.py:195-200, stops at bf16, so these have no reference counterpart - same call sites as clipa_gemm_nt:
 * the linear layers of a residual block, transformer.py:209,217-219,234, forward and input gradient).
 * clipa_quantize_rows: q[r,:] = fp8(x[r,:] * FMAX / max|x[r,:]|) (x bf16, q bytes; fmt 0 = OCP e4m3, FMAX 448; 1 = e5m2,
 * FMAX 57344), dq[r] = max|x[r,:]| / FMAX (0 for an all-zero row).  K % 8 == 0, K <= 8192.
 * clipa_gemm_nt_f8: C = epi(alpha * scale_a[m] * scale_b[n] * A8 . B8^T + bias[n]) on v_mfma_f32_16x16x128_f8f6f4, fp32
 * accumulation, bf16 C / C2 / aux and the epilogues of clipa_gemm_nt; scale_a [M], scale_b [N] may be NULL (= 1).  Whole-tile
 * shapes (M, N % 256 == 0, K % 256 == 0, K >= 512, e4m3 weights) run on the four-wave kernel of gemm_f8a.hip, bit-identical.
 * K, lda, ldb % 16 == 0 (bytes); N, ldc, ldaux % 8 == 0.  CLIPA_EPI_ACT_PRE8 / CLIPA_EPI_DACT8 (e4m3 pre-activation copy / operand, as in
 * clipa_gemm_nt; round 6) exist on the four-wave kernel only: whole-tile shapes, else CLIPA_ERR_ARG (compose GEMM + cast).
 * clipa_layernorm_fwd_q8: LayerNorm of bf16 rows emitting the e4m3 operand of the next GEMM (q, dq as quantize_rows of
 * the bf16-rounded output) and, when y != NULL, the bf16 output itself. */
int clipa_quantize_rows(const void* x, void* q, float* dq, int64_t rows, int64_t K, int64_t ldx, int64_t ldq, int fmt,
                        void* stream);
int clipa_gemm_nt_f8(const void* A8, const void* B8, const float* scale_a, const float* scale_b, void* C, void* C2,
                     const float* bias, const void* aux, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                     int64_t ldc, int64_t ldaux, float alpha, int epi, int act, int fmt_a, int fmt_b, void* stream);
int clipa_layernorm_fwd_q8(const void* x, const float* gamma, const float* beta, void* y, void* q, float* dq,
                           int64_t rows, int64_t D, float eps, void* stream);
/* Producer-fused quantisation (round 6): the fp8 operand of the next GEMM written by the kernel that produces it, with a row scale
 * the caller PREDICTS (the row maximum is spread over a row's N tiles): |sum_k a[m,k] w[n,k]| <= ||a[m,:]|| * max_n ||w[n,:]||.
 * clipa_layernorm_fwd_q8n: clipa_layernorm_fwd_q8 that also returns rownorm[r] = ||LayerNorm(x)[r,:]||_2 (bf16-rounded values).
 * clipa_gemm_nt_f8q: clipa_gemm_nt_f8 whose output C8 is e4m3 bytes (row stride ldc BYTES): row m = the bf16-rounded result times
 * scale_out[m], saturating at +-448.  epi: CLIPA_EPI_ACT (C2 NULL or the bf16 pre-activation copy), CLIPA_EPI_ACT_PRE8 (C2 = e4m3
 * pre-activation copy), CLIPA_EPI_DACT8 (aux = e4m3 bytes; colsum_partial [M / 128][N] f32 receives per-128-row column sums of the
 * UNSCALED outputs: the bias gradient after clipa_reduce_partial_rows).  Whole-tile shapes, e4m3 weights; bit-identical to
 * clipa_gemm_nt_f8 followed by clipa_scale_quantize_rows(out, scale_out, t = 1).
 * clipa_reduce_partial_rows: out[k] = sum_r partial[r][k] in a fixed order (K % 4 == 0). */
int clipa_layernorm_fwd_q8n(const void* x, const float* gamma, const float* beta, void* y, void* q, float* dq, float* rownorm,
                            int64_t rows, int64_t D, float eps, void* stream);
int clipa_gemm_nt_f8q(const void* A8, const void* B8, const float* scale_a, const float* scale_b, void* C8, void* C2,
                      const float* bias, const void* aux, const float* scale_out, float* colsum_partial, int64_t M, int64_t N,
                      int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldaux, float alpha, int epi, int act, int fmt_a,
                      void* stream);
/* CLIPA_EPI_DACT8 (C = bf16((A8 . B8^T) scale_a scale_b * act'(aux8))) that also writes the activation operand of the same layer's fp8
 * weight gradient, X8[m, n] = e4m3(act(aux8[m, n]) * scale_a[m] / t_dev[0]) (uint8 [M, ldc]) - bit for bit what
 * clipa_scale_quantize_rows_e4m3(aux8, scale_a, t_dev, ..., act) writes, from the epilogue that reads aux8 anyway.  Whole tiles only. */
int clipa_gemm_nt_f8_emit(const void* A8, const void* B8, const float* scale_a, const float* scale_b, void* C, void* X8,
                          const void* aux8, const float* t_dev, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                          int64_t ldc, int64_t ldaux, int act, int fmt_a, void* stream);
int clipa_reduce_partial_rows(const float* partial, float* out, int64_t nrows, int64_t K, void* stream);
/* The predicted row scales themselves: clipa_rownorm_max: out[0] = max_r ||w[r,:]||_2 (w bf16 [rows, K], row stride ld);
 * clipa_absmax_f32: out[0] = max |v[i]|; clipa_row_bound: bound = factor * rownorm[m] * wnorm[0] + bmax[0] (bmax NULL = 0) ->
 * scale[m] = bound / 448 (the row's de-quantisation scale), inv[m] = 448 / bound (its clipa_gemm_nt_f8q scale_out); both 0 for a
 * zero row.  wnorm / bmax are device scalars, computed once per optimizer step. */
int clipa_rownorm_max(const void* w, int64_t rows, int64_t K, int64_t ld, float* out, void* stream);
int clipa_absmax_f32(const float* v, int64_t n, float* out, void* stream);
int clipa_row_bound(const float* rownorm, const float* wnorm_dev, const float* bmax_dev, float factor, float* scale, float* inv,
                    int64_t n, void* stream);

/* fp8 WEIGHT gradients (round 6; same call sites as clipa_gemm_tn: the autograd transposes of nn.Linear / in-proj / out-proj,
 * transformer.py:209,217-219,234).  The reduction of dW = dY^T . X runs over tokens, so a per-token scale cannot be factored out:
 * P8 is the row-quantised gradient the input-gradient GEMM already consumes (clipa_quantize_rows: dY[m,:] ~ ds[m] * P8[m,:]),
 * the activation operand absorbs ds before it is quantised, Q8[m,:] = e4m3(ds[m] * X[m,:] / t), t = max_m ds[m] * sx[m] with
 * sx the activation's own row scale of the forward pass (|Q8| <= 448, nothing saturates), and dW = t * P8^T . Q8.
 * clipa_rowscale_max: out[0] = max_m a[m] * b[m] (b NULL = 1; a, b >= 0) - the scalar t, kept on the device.
 * clipa_scale_quantize_rows: q[m,:] = e4m3(act(x[m,:]) * rowscale[m] / t[0]) (act -1 = none, else the MLP activation applied and
 * rounded to bf16 first: the re-materialised gelu(h) of transformer.py:217-219); x bf16, t device scalar (0 -> zeros);
 * clipa_scale_quantize_rows_e4m3: the same with x as saturating e4m3 bytes (the kept pre-activation of CLIPA_EPI_ACT_PRE8).
 * clipa_layernorm_fwd_q8s: the same for x -> LayerNorm(x) (transformer.py:19-34; bf16-rounded as clipa_layernorm_fwd writes it).
 * clipa_gemm_tn_f8: out[R,C] = alpha * alpha_dev[0] * sum_m P8[m,R] * Q8[m,C] on v_mfma_f32_16x16x128_f8f6f4, fp32 accumulation
 * in split-M slabs + a fixed-order reduce; fmt_p 0 = e4m3 / 1 = e5m2 gradient bytes, Q8 e4m3; alpha_dev may be NULL (= 1);
 * out f32 or bf16.  R, C % 8 == 0.  Whole 256 x 256 tiles of 16-byte-aligned operands (base, ldp, ldq in bytes) run on the
 * four-wave kernel of gemm_tn8.hip; rows beyond its slices, and every other shape, on a byte-gather kernel. */
/* clipa_quantize_rows_colsum: clipa_quantize_rows that also returns colsum[k] = sum_r x[r,k] (f32 [K]) - the bias gradient of the
 * layer (the column sums of dY: nn.Linear's bias, transformer.py:209,217-219) from the pass that quantises dY for the input-gradient
 * and weight-gradient GEMMs; fixed summation order; rownorm (optional, f32 [rows]) = ||x[r,:]||_2.  workspace: per-block partial rows. */
int64_t clipa_quantize_rows_colsum_workspace(int64_t rows, int64_t K);
int clipa_quantize_rows_colsum(const void* x, void* q, float* dq, float* colsum, float* rownorm, int64_t rows, int64_t K, int64_t ldx,
                               int64_t ldq, int fmt, void* workspace, int64_t workspace_bytes, void* stream);
int clipa_rowscale_max(const float* a, const float* b, int64_t n, float* out, void* stream);
int clipa_scale_quantize_rows(const void* x, const float* rowscale, const float* t_dev, void* q, int64_t rows, int64_t K,
                              int64_t ldx, int64_t ldq, int act, void* stream);
int clipa_scale_quantize_rows_e4m3(const void* x8, const float* rowscale, const float* t_dev, void* q, int64_t rows, int64_t K,
                                   int64_t ldx, int64_t ldq, int act, void* stream);
int clipa_layernorm_fwd_q8s(const void* x, const float* gamma, const float* beta, const float* rowscale, const float* t_dev,
                            void* q, int64_t rows, int64_t D, float eps, void* stream);
int64_t clipa_gemm_tn_f8_workspace(int64_t M, int64_t R, int64_t C);
int clipa_gemm_tn_f8(const void* P8, const void* Q8, void* out, int64_t M, int64_t R, int64_t C, int64_t ldp, int64_t ldq,
                     float alpha, const float* alpha_dev, int fmt_p, int out_bf16, void* workspace, int64_t workspace_bytes,
                     void* stream);

/* F.layer_norm over the last dim, eps inside sqrt, affine (transformer.py:19-34). x/dx share a dtype
 * (x_f32), y/dy share a dtype (y_f32). bwd: dx = LN'(dy) [+ dres]; dgamma, dbeta f32 [D].
 * clipa_layernorm_bwd_y: the same backward that also writes y = LayerNorm(x) (dtype of dy), bit for bit what
 * clipa_layernorm_fwd writes - the operand of the following layer's weight gradient when a block recomputes its LayerNorm
 * outputs in backward (the reference's checkpointed block re-runs ln_1 / ln_2 there, transformer.py:238-250,320-325). */
int clipa_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, int64_t rows,
                        int64_t D, float eps, int x_f32, int y_f32, void* stream);
int64_t clipa_layernorm_bwd_workspace(int64_t rows, int64_t D);
int clipa_layernorm_bwd(const void* x, const float* gamma, const void* dy, const void* dres, void* dx,
                        float* dgamma, float* dbeta, int64_t rows, int64_t D, float eps, int x_f32,
                        int y_f32, void* workspace, int64_t workspace_bytes, void* stream);
int clipa_layernorm_bwd_y(const void* x, const float* gamma, const float* beta, const void* dy, const void* dres, void* dx,
                          void* y, float* dgamma, float* dbeta, int64_t rows, int64_t D, float eps, int x_f32,
                          int y_f32, void* workspace, int64_t workspace_bytes, void* stream);
/* fp8 engine (no reference counterpart, as the clipa_quantize_rows family above): the bf16 LayerNorm backward that also hands
 * the linear layer in front of it its incoming gradient as fp8 operand - q uint8 [rows, D] (fmt 0 = e4m3, 1 = e5m2), dq f32 [rows]
 * (bit for bit what clipa_quantize_rows makes of the bf16 dx this call writes), colsum f32 [D] = sum over rows of dx (that
 * layer's bias gradient), rownorm f32 [rows] (optional: ||dx[r,:]||_2).  beta / y: NULL, or both given as in clipa_layernorm_bwd_y. */
int64_t clipa_layernorm_bwd_q8_workspace(int64_t rows, int64_t D);
int clipa_layernorm_bwd_q8(const void* x, const float* gamma, const float* beta, const void* dy, const void* dres, void* dx, void* y,
                           void* q, float* dq, float* colsum, float* rownorm, float* dgamma, float* dbeta, int64_t rows, int64_t D,
                           float eps, int fmt, void* workspace, int64_t workspace_bytes, void* stream);

/* softmax(q.k^T * scale + mask).v per (batch, head); q/k/v are column blocks of the packed projection
 * output (row stride ld_qkv), out is [B*L, H*dh] (row stride ld_o). causal = additive triu(1)*-inf mask.
 * Replaces F.scaled_dot_product_attention inside nn.MultiheadAttention (transformer.py:223-236). */
/* stats (optional in fwd, required in bwd): f32 [B*H*L][2] = (scale*log2(e)*rowmax, 1/rowsum) of the softmax. */
int clipa_attention_fwd(const void* q, const void* k, const void* v, void* out, float* stats, int64_t B,
                        int64_t H, int64_t L, int64_t dh, int64_t ld_qkv, int64_t ld_o, float scale,
                        int causal, void* stream);
int clipa_attention_bwd(const void* q, const void* k, const void* v, const void* out, const void* d_out,
                        const float* stats, void* dq, void* dk, void* dv, int64_t B, int64_t H, int64_t L,
                        int64_t dh, int64_t ld_qkv, int64_t ld_o, int64_t ld_dqkv, float scale, int causal,
                        void* stream);
/* The same kernels on PACKED variable-length sequences (MI355X engine extension: the text tower on the tokens up to each
 * caption's EOT - under the causal mask of transformer.py:618-624 no later position can reach the pooled output of
 * model.py:251-254 or receive gradient, so features, loss and gradients are unchanged).  q / k / v / out rows are token rows of
 * the packed matrix; sequence s occupies rows [seq_start[s], seq_start[s] + seq_len[s]).  One call processes the nseq
 * sequences named by seq_ids (int32 device array; NULL = sequences 0 .. nseq-1), all of length <= 32 * tiles (tiles <= 9);
 * stats: T * H (max, 1/sum) pairs.  Head dims 64 / 80. */
int clipa_attention_fwd_varlen(const void* q, const void* k, const void* v, void* out, float* stats,
                               const int32_t* seq_start, const int32_t* seq_len, const int32_t* seq_ids, int64_t nseq,
                               int64_t tiles, int64_t H, int64_t dh, int64_t ld_qkv, int64_t ld_o, float scale, int causal,
                               void* stream);
int clipa_attention_bwd_varlen(const void* q, const void* k, const void* v, const void* out, const void* d_out,
                               const float* stats, void* dq, void* dk, void* dv, const int32_t* seq_start,
                               const int32_t* seq_len, const int32_t* seq_ids, int64_t nseq, int64_t tiles, int64_t H, int64_t dh,
                               int64_t ld_qkv, int64_t ld_o, int64_t ld_dqkv, float scale, int causal, void* stream);

/* image [B,3,S,S] (or NHWC) u8/bf16/f32 -> bf16 patch matrix [B*(S/P)^2, Kp], elements in (ph,pw,c)
 * order, optional (x/255 - mean)/std (train.py:191-197 + conv1 im2col, transformer.py:371,491-493). */
int clipa_patchify(const void* img, void* out, int64_t B, int64_t S, int64_t P, int64_t Kp, int in_dtype,
                   int nhwc, int normalize, const float* mean3, const float* std3, void* stream);
/* Device-side train transform on uint8 NHWC batches (replaces the per-sample CPU work of
 * open_clip/transform.py:152-168 after the H2D copy of training/train.py:187-189): out[b] = Grayscale?(resize(crop(src[b],
 * box[b]), S x S, BICUBIC)) bit-exact with Pillow's ImagingResample / rgb2l (what torchvision's RandomResizedCrop and
 * Grayscale(3) run on PIL images).  src [B,Hs,Ws,3], out [B,S,S,3]; boxes int32 [B][4] = (top, left, height, width), sampled
 * by the caller; gray_flags uint8 [B] or NULL; err_count (device int32, may be NULL) counts rejected samples (box outside the
 * image, or a down-scale above 11x) whose output is zeros. */
int64_t clipa_resized_crop_workspace(int64_t B, int64_t Hs, int64_t S);
int clipa_resized_crop_u8(const void* src, const int32_t* boxes, const uint8_t* gray_flags, void* out, int64_t B, int64_t Hs,
                          int64_t Ws, int64_t S, void* workspace, int64_t workspace_bytes, int32_t* err_count, void* stream);
/* torchvision ColorJitter (per-sample op order[b][0..3] over {0 brightness, 1 contrast, 2 saturation, 3 hue}, factors[b][op];
 * samples with apply[b] == 0 are left alone; order == NULL skips the jitter) followed by Grayscale(3) of the samples flagged in
 * gray_flags (NULL: none), IN PLACE on uint8 [B,S,S,3] - the color_jitter / gray_scale stages of open_clip/transform.py:61-84,
 * 160-168, bit-exact with the Pillow code they run on PIL images.  workspace: 8 bytes per sample. */
int clipa_color_jitter_u8(void* img, const uint8_t* apply, const int32_t* order, const float* factors, const uint8_t* gray_flags,
                          int64_t B, int64_t S, void* workspace, int64_t workspace_bytes, void* stream);
/* The same resampler on a RAGGED batch - every sample its own source size - and with the inference geometry: replaces the
 * per-sample CPU work of the train transform (open_clip/transform.py:152-168) for images of mixed sizes and of the eval
 * transform, Resize(S, bicubic | bilinear) + CenterCrop(S) or Resize((S, S)) (open_clip/transform.py:186-213; --interpolation,
 * --square-resize-only of training/params.py:445-454):
 *   out[b][y][x] = Grayscale?(resize(crop(img_b, box_b), (out_h_b, out_w_b), filter))[oy_b + y][ox_b + x],  0 <= y, x < S
 * bit-exact with Pillow's ImagingResample.  img_b is H_b x W_b x 3 uint8 at byte offset off_b of `packed` (packed_bytes long);
 * out is uint8 [B,S,S,3]; filter 0 bicubic, 1 bilinear.  desc is int64 [B][16] on the device: off, H, W, box top, left,
 * height, width, out_h, out_w, oy, ox, then the sample's storage, laid out by the host from the size table: byte offset of its
 * intermediate rows in the tmp_bytes region, int offset of its coefficient tables in the coef_ints region (S x kh horizontal,
 * then S x kv vertical), kh, kv (taps per output coordinate, >= 2 * ceil(support * max(1, in / out)) + 1) and the number of
 * intermediate rows reserved; max_rows = the largest such number.  Every descriptor is validated on the device before it is
 * dereferenced (image inside [packed, packed + packed_bytes), box inside the image, window inside the resized image, sides
 * <= 16384, down-scale <= 64x per axis, storage inside the workspace): a failing sample is counted in err_count (device
 * int32, may be NULL) and its output is zeros. */
int64_t clipa_resample_ragged_workspace(int64_t B, int64_t S, int64_t tmp_bytes, int64_t coef_ints);
int clipa_resample_ragged_u8(const void* packed, int64_t packed_bytes, const int64_t* desc, const uint8_t* gray_flags, void* out,
                             int64_t B, int64_t S, int filter, int64_t max_rows, int64_t tmp_bytes, int64_t coef_ints,
                             void* workspace, int64_t workspace_bytes, int32_t* err_count, void* stream);
/* cat(class_embedding) + positional_embedding (transformer.py:496-499) and its gradient. */
int clipa_assemble_tokens(const void* patch, const float* cls, const float* pos, void* tokens, int64_t B,
                          int64_t L, int64_t D, void* stream);
/* the batch sums (dcls, dpos) go through per-chunk partials in `workspace` and a fixed-order reduce: bit-reproducible */
int64_t clipa_assemble_tokens_bwd_workspace(int64_t B, int64_t L, int64_t D);
int clipa_assemble_tokens_bwd(const void* dtokens, void* dpatch, float* dcls, float* dpos, int64_t B,
                              int64_t L, int64_t D, void* workspace, int64_t workspace_bytes, void* stream);
/* token_embedding(text) + positional_embedding (model.py:245-247) and gradients (dense f32 table grad). */
int clipa_embed_tokens(const int64_t* ids, const void* table, int table_bf16, const float* pos, void* out,
                       int64_t B, int64_t T, int64_t D, int64_t vocab, int32_t* oob_count, void* stream);
/* oob_count (device int32, may be NULL): incremented once per token id outside [0, vocab) - nn.Embedding raises on
 * those; the forward substitutes row 0, the backward skips the row, the caller turns a non-zero count into an error
 * (clipa_amd.ops checks it asynchronously). */
/* The table gradient is a scatter-add on 64-bit fixed-point accumulators in `workspace` (integer atomics commute: the
 * result is bit-reproducible), converted to f32 at the end; dpos goes through clipa_assemble_tokens_bwd's ordered sums. */
int64_t clipa_embed_tokens_bwd_workspace(int64_t B, int64_t T, int64_t D, int64_t vocab, int need_table, int need_pos);
int clipa_embed_tokens_bwd(const int64_t* ids, const void* dx, float* dtable, float* dpos, int64_t B,
                           int64_t T, int64_t D, int64_t vocab, int32_t* oob_count, void* workspace,
                           int64_t workspace_bytes, void* stream);
/* text.argmax(dim=-1) (model.py:254) */
int clipa_argmax_tokens(const int64_t* ids, int32_t* out, int64_t B, int64_t T, void* stream);
/* pooling [B,L,D] bf16 -> [B,D] f32 and its gradient (writes all of dx) */
int clipa_pool_fwd(const void* x, const int32_t* idx, float* out, int64_t B, int64_t L, int64_t D, int mode,
                   void* stream);
int clipa_pool_bwd(const float* dout, const int32_t* idx, void* dx, int64_t B, int64_t L, int64_t D,
                   int mode, void* stream);
/* PatchDropout (transformer.py:53-83,501-502): the kept tokens as a row selection of the bf16 token matrix.
 * gather: out[r,:] = x[rows[r],:] (r < n_out; rows outside [0, n_src) read zeros); scatter = its backward:
 * dx[n_dst, D] = 0, dx[rows[r],:] = dy[r,:] (rows distinct).  rows: int64 on the device.  D % 8 == 0. */
int clipa_gather_rows(const void* x, const int64_t* rows, void* out, int64_t n_out, int64_t n_src, int64_t D,
                      void* stream);
int clipa_scatter_rows(const void* dy, const int64_t* rows, void* dx, int64_t n_src, int64_t n_dst, int64_t D,
                       void* stream);
/* F.normalize(x, dim=-1) (model.py:240,263); y_bf16 optional second output */
int clipa_l2norm_fwd(const float* x, float* y, void* y_bf16, float* inv_norm, int64_t rows, int64_t E,
                     float eps, void* stream);
int clipa_l2norm_bwd(const float* y, const float* inv_norm, const float* dy, float* dx, int64_t rows,
                     int64_t E, void* stream);
/* bias gradients: out[n] = sum_m dY[m,n] */
int64_t clipa_colsum_workspace(int64_t M, int64_t N);
int clipa_colsum(const void* dy, float* out, int64_t M, int64_t N, int64_t ld, void* workspace,
                 int64_t workspace_bytes, void* stream);
/* dtype / layout plumbing for weights */
int clipa_cast_to_bf16(const void* in, int in_f32, void* out, int64_t n, void* stream);
int clipa_cast_bf16_to_f32(const void* in, float* out, int64_t n, void* stream);
int clipa_transpose_to_bf16(const void* in, int in_f32, void* out, int64_t R, int64_t C, int64_t ldi,
                            int64_t ldo, void* stream);
/* LayerScale (open_clip/transformer.py:43-50, applied at :248-249: x + gamma * (a W^T + b)) folded into the layer it scales,
 * so that the GEMMs run unchanged on W' = diag(gamma) W and b' = gamma * b.  w [N,K] bf16 or f32 (w_f32), gamma / b f32 [N].
 * fold:   w_folded [N,K] bf16 = bf16(gamma[n] * w[n,k]) (fp32 product, one rounding), b_folded f32 [N] = gamma * b.
 * unfold: from dw_folded f32 [N,K] = dY^T X and db_folded f32 [N] = colsum(dY) of the folded layer:
 *         dw [N,K] (f32 if dw_f32, else bf16) = gamma[n] * dw_folded[n,k], db f32 = gamma * db_folded,
 *         dgamma f32 [N] = sum_k dw_folded[n,k] * w[n,k] + db_folded[n] * b[n]  (fp32, fixed summation order, no atomics).
 *         A null dw / db / dgamma skips that output (frozen parameter).
 * Any K: rows that are not 16-byte aligned (K % 8 != 0, unaligned bases) take a scalar path. */
int clipa_layerscale_fold(const void* w, int w_f32, const float* gamma, const float* b, void* w_folded, float* b_folded,
                          int64_t N, int64_t K, void* stream);
int clipa_layerscale_unfold(const float* dw_folded, const void* w, int w_f32, const float* gamma, const float* db_folded,
                            const float* b, void* dw, int dw_f32, float* db, float* dgamma, int64_t N, int64_t K,
                            void* stream);
/* Dual PatchNorm stem (input_patchnorm, arXiv 2302.01327; open_clip/transformer.py:362-371,483-489: rearrange to
 * [B, g*g, 3*P*P], patchnorm_pre_ln = LayerNorm(3*P*P, eps 1e-5), conv1 = nn.Linear(3*P*P, width)).  K = 3*P*P.
 * patchify_ln: clipa_patchify's inputs and geometry (Kp % 8 == 0, 3*P*P <= Kp <= 3072, pixels beyond g*P never read) ->
 *         bf16 [B*g*g, Kp] = (x - mean) * rstd of every patch row, WITHOUT the affine; columns in (ph,pw,c) order, columns
 *         >= K zero.  fp32 statistics over the K real elements (mean first, then the centred sum of squares), taken on the row
 *         minus its first element: a constant patch gives exact zeros.  One wave per patch row, the row in registers.
 * fold:   gamma / beta f32 [K] of the LayerNorm and w [N,K] (bf16, or f32 if w_f32) / b f32 [N] of the Linear, all in the
 *         parameters' (c,p1,p2) column order -> w_folded bf16 [N,Kp] = bf16(w[n,k] * gamma[k]) (fp32 product, one rounding)
 *         with the columns permuted to (ph,pw,c) and zero padding, b_folded f32 [N] = b[n] + sum_k w[n,k] * beta[k] (fp32,
 *         fixed order): LayerNorm_K(x) W^T + b == xhat w_folded^T + b_folded.
 * unfold: from g f32 [N,Kp] = dPE^T xhat (columns in (ph,pw,c) order) and s f32 [N] = colsum(dPE):
 *         dw [N,K] (f32 if dw_f32, else bf16; (c,p1,p2) order) = gamma[k] * g[n,k] + beta[k] * s[n],
 *         dgamma f32 [K] = sum_n w[n,k] * g[n,k], dbeta f32 [K] = sum_n w[n,k] * s[n] (fp32, fixed summation order over n, no
 *         atomics).  A null dw / dgamma / dbeta skips that output (frozen parameter).  The bias gradient is s itself. */
int clipa_patchify_ln(const void* img, void* out, int64_t B, int64_t S, int64_t P, int64_t Kp, int in_dtype, int nhwc,
                      int normalize, const float* mean3, const float* std3, float eps, void* stream);
int clipa_patchnorm_fold(const void* w, int w_f32, const float* b, const float* gamma, const float* beta, void* w_folded,
                         float* b_folded, int64_t N, int64_t P, int64_t Kp, void* stream);
int clipa_patchnorm_unfold(const float* g, const float* s, const void* w, int w_f32, const float* gamma, const float* beta,
                           void* dw, int dw_f32, float* dgamma, float* dbeta, int64_t N, int64_t P, int64_t Kp, void* stream);
/* out = act(in) elementwise, bf16 (MLP activation re-materialised from the kept pre-activation) */
int clipa_activation_fwd(const void* in, void* out, int64_t n, int act, void* stream);
/* Fused similarity + cross-entropy of the InfoNCE loss (loss.py:128-155): logits = s * rows . cols^T (rows [R,E],
 * cols [N,E] bf16, s = exp(logit_scale) read from DEVICE memory, NULL = 1), labels label0 + r.  The [R,N] fp32 logits are
 * never written: the forward GEMM's epilogue keeps per-tile (max, sum exp) partials, merged into lse[R] and
 * loss_rows[R] = lse - logit[label]; the backward re-runs the GEMM and writes the bf16 gradient
 * d loss / d (rows.cols^T) = s * gscale * (softmax - onehot) ([R, ldd], ldd >= N rounded up to 8, pad columns zero) plus
 * dscale_rows[R] = per-row d loss / d s.  Workspace: clipa_simce_workspace(R, N) bytes for either call. */
int64_t clipa_simce_workspace(int64_t R, int64_t N);
int clipa_simce_fwd(const void* rows, const void* cols, int64_t R, int64_t N, int64_t E, int64_t lda, int64_t ldb,
                    const float* scale, int64_t label0, float* lse, float* loss_rows, void* workspace,
                    int64_t workspace_bytes, void* stream);
int clipa_simce_bwd(const void* rows, const void* cols, int64_t R, int64_t N, int64_t E, int64_t lda, int64_t ldb,
                    const float* scale, int64_t label0, float gscale, const float* lse, void* dlogits_bf16,
                    int64_t ldd, float* dscale_rows, void* workspace, int64_t workspace_bytes, void* stream);
/* Fused similarity + cross-entropy + distillation loss of DistillClipLoss (loss.py:202-238), one direction: student
 * logits z = s * rows_s . cols_s^T ([R,E_s] . [N,E_s]^T), teacher logits y = u * rows_t . cols_t^T ([R,E_t] . [N,E_t]^T),
 * bf16 operands, s and u read from DEVICE memory (NULL = 1), labels label0 + r.  Forward: lse_s[R], lse_t[R],
 * ce_rows[R] = lse_s - z[label], dist_rows[R] = lse_s - sum_j softmax(y)_j z_j; neither logit matrix is written.
 * Backward: the bf16 d loss / d (rows_s . cols_s^T) = s * gscale * (g_c (p^s - onehot) + g_d (p^s - p^t)) ([R, ldd],
 * ldd >= N rounded up to 8, pad columns zero) plus dscale_rows[R] = per-row d loss / d s; g_c, g_d are DEVICE scalars
 * (NULL = 1), the teacher gets no gradient.  Workspace: clipa_simce_distill_workspace(R, N) bytes for either call. */
int64_t clipa_simce_distill_workspace(int64_t R, int64_t N);
int clipa_simce_distill_fwd(const void* rows_s, const void* cols_s, const void* rows_t, const void* cols_t, int64_t R,
                            int64_t N, int64_t Es, int64_t Et, int64_t ldas, int64_t ldbs, int64_t ldat, int64_t ldbt,
                            const float* scale_s, const float* scale_t, int64_t label0, float* lse_s, float* lse_t,
                            float* ce_rows, float* dist_rows, void* workspace, int64_t workspace_bytes, void* stream);
int clipa_simce_distill_bwd(const void* rows_s, const void* cols_s, const void* rows_t, const void* cols_t, int64_t R,
                            int64_t N, int64_t Es, int64_t Et, int64_t ldas, int64_t ldbs, int64_t ldat, int64_t ldbt,
                            const float* scale_s, const float* scale_t, int64_t label0, float gscale, const float* g_c,
                            const float* g_d, const float* lse_s, const float* lse_t, void* dlogits_bf16, int64_t ldd,
                            float* dscale_rows, void* workspace, int64_t workspace_bytes, void* stream);
/* Fused similarity + pairwise sigmoid loss of SigLIP (the element maths of clipa_jax/losses/common.py:25-32, sigmoid_xent):
 * l = s * rows . cols^T + b (rows [R,E], cols [N,E] bf16; s and b read from DEVICE memory, both required), y = +1 at column
 * label0 + r and -1 elsewhere, t = y * l.  ONE pass over the GEMM: loss_rows[R] = sum_n softplus(-t) (not scaled by gscale),
 * and - unless the three gradient pointers are all NULL (forward only) - with gg = gscale * (-y) * sigmoid(-t): the bf16
 * d loss / d (rows.cols^T) = gg * s ([R, ldd], N rounded up to 8 <= ldd <= N rounded up to 256, columns [N, ldd) zero),
 * dscale_rows[R] = sum_n gg * (rows.cols^T) and dbias_rows[R] = sum_n gg.  The [R,N] logits are never written.
 * Workspace: clipa_simsig_workspace(R, N) bytes. */
int64_t clipa_simsig_workspace(int64_t R, int64_t N);
int clipa_simsig(const void* rows, const void* cols, int64_t R, int64_t N, int64_t E, int64_t lda, int64_t ldb,
                 const float* scale, const float* bias, int64_t label0, float gscale, float* loss_rows,
                 void* dlogits_bf16, int64_t ldd, float* dscale_rows, float* dbias_rows, void* workspace,
                 int64_t workspace_bytes, void* stream);
/* Multihead attention pooling, the "map" head of clipa_jax/models/vit.py:187-207, token-level part.  The head has one
 * learned query for every sample, so the K / V projections fold out: with U[H,D] = dh^-0.5 Wk_h^T q_h (bf16),
 * s[b,l,h] = x[b,l,:] . U[h,:], p = softmax over l, z[b,h,:] = sum_l p[b,l,h] x[b,l,:].  x bf16 [B*L, ldx] (ldx >= D, a
 * multiple of 8), read once.  fwd -> z f32 [B,H,D], stats f32 [B,H,2] (row max, sum of exp).  bwd (clipa_jax/models/
 * vit.py:187-207 differentiated through the same fold): from x, U, z, stats and dz f32 [B,H,D] -> dx bf16 [B*L, lddx]
 * (every row written once) and dU f32 [H,D], summed over per-workgroup partials in a fixed order (no atomics: bit-identical
 * from run to run at a given B and max_workgroups).  P, dS and dz are rounded to bf16 as MFMA operands.  1 <= H <= 16,
 * D % 64 == 0, 64 <= D <= 2048, L >= 1; B <= 0 returns OK (bwd: dU = 0).  max_workgroups <= 0: the library's default.
 * Workspace (bwd): clipa_mappool_bwd_workspace(B, H, D, max_workgroups) bytes.  Pointers 16-byte aligned. */
int64_t clipa_mappool_bwd_workspace(int64_t B, int64_t H, int64_t D, int64_t max_workgroups);
int clipa_mappool_fwd(const void* x, const void* U, float* z, float* stats, int64_t B, int64_t L, int64_t D, int64_t H,
                      int64_t ldx, int64_t max_workgroups, void* stream);
int clipa_mappool_bwd(const void* x, const void* U, const float* z, const float* stats, const float* dz, void* dx, float* dU,
                      int64_t B, int64_t L, int64_t D, int64_t H, int64_t ldx, int64_t lddx, int64_t max_workgroups,
                      void* workspace, int64_t workspace_bytes, void* stream);
int clipa_sum_scale(const float* in, float* out, int64_t n, float scale, int accumulate, void* stream);
/* Retrieval ranks of the validation metrics (get_clip_metrics, clipa_torch/training/train.py:432-449) without the [N, N]
 * logit matrix.  A (image features) and B (text features) are fp32 [N, E] with leading dimensions lda, ldb (>= E, multiples
 * of 4), row i of each a matched pair; s is read from DEVICE memory (NULL = 1).  With v_ij = fl(s * (A_i . B_j)), every x_ij
 * computed by the same fp32 arithmetic (one ascending-k fmaf chain per output, the diagonal included):
 *   i2t_gt[i] = #{j != i : v_ij > v_ii}   i2t_eq[i] = #{j != i : v_ij == v_ii}   (row i, image -> text)
 *   t2i_gt[j] = #{i != j : v_ij > v_jj}   t2i_eq[j] = #{i != j : v_ij == v_jj}   (column j, text -> image)
 * Tie rule: the reference's 0-based position of the positive after an unstable descending argsort is some value in
 * [gt, gt + eq]; gt is the optimistic, deterministic choice the engine reports.  All pointers 16-byte aligned (scale 4);
 * the count arrays need no clearing.  Workspace: clipa_retrieval_ranks_workspace(N) bytes.  Memory is O(N). */
int64_t clipa_retrieval_ranks_workspace(int64_t N);
int clipa_retrieval_ranks(const float* A, const float* B, int64_t N, int64_t E, int64_t lda, int64_t ldb,
                          const float* scale, int32_t* i2t_gt, int32_t* i2t_eq, int32_t* t2i_gt, int32_t* t2i_eq,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* Multi-caption image-text retrieval ranks (clipa_jax/evaluators/proj/image_text/image_text_retrieval.py: COCO, Flickr30k)
 * without the [Ni, Nt] similarity matrix.  A (image features) fp32 [Ni, E], B (text features) fp32 [Nt, E], leading
 * dimensions lda, ldb (>= E, multiples of 4); txt2img int32 [Nt] in DEVICE memory, text t describing image c(t) in
 * [0, Ni) (callers validate it; the kernels never index with it); s from DEVICE memory (NULL = 1).  With
 * v_it = fl(s * (A_i . B_t)), every x_it computed by the same fp32 arithmetic as clipa_retrieval_ranks:
 *   p_t = v_{c(t), t}   m_i = max over {t : c(t) = i} of p_t   (-inf when image i has no caption)
 *   t2i_gt[t] = #{i : v_it > p_t}   t2i_eq[t] = #{i != c(t) : v_it == p_t}          (text -> image)
 *   i2t_gt[i] = #{t : v_it > m_i}   i2t_eq[i] = #{t : c(t) != i, v_it == m_i}       (image -> text)
 * i2t_gt is the 0-based position of image i's best caption (Nt for a captionless image), t2i_gt that of text t's image;
 * tie rule as clipa_retrieval_ranks.  Any c is correct; c non-decreasing (the captions of an image adjacent) makes the
 * positives pass touch about Ti + Tt 128 x 128 tiles instead of up to Ti * Tt.  All pointers 16-byte aligned (scale 4);
 * the count arrays need no clearing.  Workspace: clipa_retrieval_ranks_multi_workspace(Ni, Nt) bytes.  Memory is
 * O(Ni + Nt). */
int64_t clipa_retrieval_ranks_multi_workspace(int64_t Ni, int64_t Nt);
int clipa_retrieval_ranks_multi(const float* A, const float* B, const int32_t* txt2img, int64_t Ni, int64_t Nt, int64_t E,
                                int64_t lda, int64_t ldb, const float* scale, int32_t* i2t_gt, int32_t* i2t_eq,
                                int32_t* t2i_gt, int32_t* t2i_eq, void* workspace, int64_t workspace_bytes, void* stream);
/* Few-shot linear probe (clipa_jax/evaluators/fewshot_lsr.py, big_vision's closed-form L2-regularised least squares on frozen
 * features).  Everything fp32; every reduction in a fixed order (no float atomics, results bit-reproducible); pointers 16-byte
 * aligned (index 4), matrices row-major.  Zero-sized inputs return CLIPA_OK with the result of the empty computation: no
 * output where there is nothing to write; moments over N = 0 rows gives mean = std = NaN (0 / 0, as numpy); gram over E = 0
 * columns gives S = 0; predict over dim = 0 gives pred = 0, best = 0.  The one exception is predict with C = 0 classes for
 * Nt > 0 rows, CLIPA_ERR_ARG: no argmax exists.
 * moments (fewshot_lsr.py:39-40): over rows index[0..N) of x [Ntot, D] (index NULL: rows 0..N), mean[d] and
 * std[d] = sqrt(mean((x - mean)^2)) + 1e-5 in two passes.  An index outside [0, Ntot) is never dereferenced (its row reads NaN). */
int clipa_fewshot_moments(const float* x, const int32_t* index, int64_t N, int64_t Ntot, int64_t D, int64_t ldx, float* mean,
                          float* std, void* stream);
/* whiten (fewshot_lsr.py:41-44, 95-96): Z [N, ldz] = (x[index] - mean) / std (a true subtraction, then a true division), column
 * D = 100.0 (BIAS_CONSTANT), columns (D, ldz) = 0; ldz >= D + 1.  Zt (optional) [D + 1, ldt] = the transpose, columns [N, ldt) = 0. */
int clipa_fewshot_whiten(const float* x, const int32_t* index, int64_t N, int64_t Ntot, int64_t D, int64_t ldx,
                         const float* mean, const float* std, float* Z, int64_t ldz, float* Zt, int64_t ldt, void* stream);
/* gram (x.T @ x / x @ x.T of fewshot_lsr.py:72-79): S [M, lds] = A A^T for A [M, E] (lda >= E, a multiple of 4), one ascending-k
 * fp32 fmaf chain per entry (the arithmetic of clipa_retrieval_ranks), the upper 128 x 128 tiles computed and mirrored:
 * S == S^T bit for bit. */
int clipa_fewshot_gram(const float* A, int64_t M, int64_t E, int64_t lda, float* S, int64_t lds, void* stream);
/* class sums (x.T @ y of fewshot_lsr.py:47, 74 for y = +1 at the label, -1 elsewhere, y never formed): the rows of Z [N, ldz]
 * sorted by class, offsets int32 [C + 1] in DEVICE memory (class c = rows [offsets[c], offsets[c + 1]), clamped to [0, N]);
 * R [dim, ldr], R[d, c] = 2 sum_{n in c} Z[n, d] - sum_n Z[n, d]: segment sums in row order, their total in class order.
 * C <= 65535. */
int clipa_fewshot_class_sums(const float* Z, const int32_t* offsets, int64_t N, int64_t dim, int64_t C, int64_t ldz, float* R,
                             int64_t ldr, void* stream);
/* predict (jnp.argmax(x_test @ w, axis=1), fewshot_lsr.py:107) without the [Nt, C] logits: Z [Nt, ldz] whitened test rows,
 * W [C, ldw] class-major weights (ldz, ldw >= dim, multiples of 4), logits by the arithmetic of clipa_fewshot_gram;
 * pred[n] = the lowest class index among the maxima of row n, best[n] = that logit (finite logits assumed). */
int clipa_fewshot_predict(const float* Z, const float* W, int64_t Nt, int64_t C, int64_t dim, int64_t ldz, int64_t ldw,
                          int32_t* pred, float* best, void* stream);
/* Logistic-regression linear probe (Radford et al. 2021, "Learning Transferable Visual Models From Natural Language
 * Supervision", section 3.2 and appendix A.3: an L2-regularised multinomial logistic regression on frozen image features, fitted
 * with L-BFGS; the reference has no such evaluator, so the paper is cited where its lines would be).  One objective-and-gradient
 * evaluation at theta [C, dim], dim = D + 1, class-major, the last column the bias; x~_n = [x_n, 1]:
 *   f_data = (1 / N) sum_n (lse_n - z_{n, y_n}),  z_n = theta x~_n,  lse_n = log sum_c exp z_{n, c}        (A.3)
 *   d f_data / d theta = (1 / N) (softmax(z) - onehot(y))^T X~
 * The kernels compute the sums; the 1 / N, the sum over n of ce and the L2 term are the caller's (fp64 on the host).  Everything
 * fp32, every reduction in a fixed order (no float atomics: results bit-reproducible whatever the grid); pointers 16-byte
 * aligned, matrices row-major, leading dimensions multiples of 4.  N < 2^21 (a 128-class block of the [C, N] logits stays below
 * 1 GiB), C <= 65535, dim < 2^21; CLIPA_ERR_ARG with a message otherwise.  Zero sizes return CLIPA_OK where the result is empty
 * (N = 0 for prepare, logits and residual; C = 0 or dim = 0 for grad; grad over N = 0 samples gives dtheta = 0); C = 0 with
 * N > 0 is CLIPA_ERR_ARG for logits and residual.
 * prepare: Xp [N, ld] = [x, 1] with columns (D, ld) = 0, and Xt [D + 1, ldn] = its transpose with columns [N, ldn) = 0; x [N, ldx],
 * ld >= D + 1, ldn >= N.  Once per fit. */
int clipa_logreg_prepare(const float* x, int64_t N, int64_t D, int64_t ldx, float* Xp, int64_t ld, float* Xt, int64_t ldn,
                         void* stream);
/* logits: Zt [C, ldz >= N], Zt[c, n] = theta_c . x~_n by the arithmetic of clipa_fewshot_gram (theta [C, ldt], Xp [N, ld] of
 * prepare), columns [N, ldz) untouched; lse[n] = log sum_c exp Zt[c, n]; pred[n] = the lowest class among the maxima of column
 * n, best[n] = that logit (both equal clipa_fewshot_predict on the same operands bit for bit).  lse keeps, per sample and
 * 128-class tile, a running (m, s): m' = max(m, max_c v_c), s = s exp(m - m') + sum_c exp(v_c - m') with c ascending inside a
 * lane's 32 classes of the tile, expf / logf; the 4 partial results of a sample meet in a fixed order. */
int clipa_logreg_logits(const float* theta, const float* Xp, int64_t C, int64_t N, int64_t dim, int64_t ldt, int64_t ld, float* Zt,
                        int64_t ldz, float* lse, int32_t* pred, float* best, void* stream);
/* residual: ce[n] = lse[n] - Zt[y_n, n] (the sample's cross entropy), then, with overwrite != 0, in place
 * Zt[c, n] <- expf(Zt[c, n] - lse[n]) - [c == y_n] (softmax minus one-hot: Gt).  overwrite = 0 writes ce alone (a line-search
 * probe).  y int32 [N] in DEVICE memory; a label outside [0, C) gives ce[n] = NaN and is not used as an index. */
int clipa_logreg_residual(float* Zt, const float* lse, const int32_t* y, int64_t C, int64_t N, int64_t ldz, float* ce,
                          int32_t overwrite, void* stream);
/* grad: dtheta [C, ldg >= dim], dtheta[c, d] = sum_n Gt[c, n] Xt[d, n] (Gt [C, ldz] of residual, Xt [dim, ldn] of prepare),
 * columns [dim, ldg) untouched.  n is cut into slices of `slice` samples (0: the default 4096; a multiple of 4 - a constant of
 * the algorithm, not of the launch: another value changes the last bits); each slice's product is one ascending-n fp32 chain
 * per entry, and the slices' partials are added in ascending order.  max_workgroups (0: no limit) caps the grid and changes no
 * bit.  Workspace: clipa_logreg_grad_workspace(C, dim, N, slice) bytes (0 for a single slice). */
int64_t clipa_logreg_grad_workspace(int64_t C, int64_t dim, int64_t N, int64_t slice);
int clipa_logreg_grad(const float* Gt, const float* Xt, int64_t C, int64_t dim, int64_t N, int64_t ldz, int64_t ldn,
                      float* dtheta, int64_t ldg, int64_t slice, int64_t max_workgroups, void* workspace,
                      int64_t workspace_bytes, void* stream);
/* Zero-shot classification (clipa_torch/training/zero_shot.py:29-90; clipa_jax/evaluators/proj/image_text/
 * discriminative_classifier.py:152-171, 302-312).  Everything fp32, every reduction in a fixed order (no float atomics, results
 * bit-reproducible); pointers 16-byte aligned, matrices row-major.
 * class mean (zero_shot.py:37-38; _average_embeddings, discriminative_classifier.py:165-170): the rows of emb [N, lde] sorted by
 * class, offsets int32 [C + 1] in DEVICE memory (class c = rows [offsets[c], offsets[c + 1]), clamped to [0, N]); W [C, ldw],
 * W_c = m_c / (eps + ||m_c||) with m_c the mean of the rows of class c, columns [E, ldw) = 0; lde, ldw >= E.  eps = 0 is the
 * torch reference (inputs already unit-norm), eps = 1e-8 the JAX one.  One accumulator per (class, column) in ascending row
 * order, true division and square root; the order of the sum of squares is in csrc/zeroshot.hip.  An empty class has no mean
 * ("Classes without embeddings", :164): N < C is CLIPA_ERR_ARG, and a caller checks its offsets before the call - the row of
 * an empty class comes out NaN.  C = 0 returns CLIPA_OK without a launch. */
int clipa_zeroshot_class_mean(const float* emb, const int32_t* offsets, int64_t N, int64_t C, int64_t E, int64_t lde, float eps,
                              float* W, int64_t ldw, void* stream);
/* ranks (replaces logits = 100 * f @ classifier and accuracy's topk, zero_shot.py:47-50, 77-80, and best_txt / matching of
 * discriminative_classifier.py:303-309) without the [B, C] logits: A [B, lda] image features, W [C, ldw] classifier (lda,
 * ldw >= E, multiples of 4), labels int32 [B, Lmax] (1 <= Lmax <= 32, -1 = no label; a value outside [0, C) names no class).
 * v_ic = A_i . W_c by the arithmetic of clipa_retrieval_ranks (one ascending-k fp32 chain, no scale: the reference's 100 *
 * changes no order but can merge neighbours).  t_i = max over i's labels of v_ic;
 * gt[i] = #{c : v_ic > t_i}, eq[i] = #{c not a label of i : v_ic == t_i}, pred[i] = the lowest class index among the maxima of
 * row i.  A row without labels gets gt = C, eq = 0.  Finite inputs assumed.  O(B + C E) memory, no workspace, plain stores.
 * B = 0 returns CLIPA_OK without a launch; B > 0 with C = 0 or E = 0 is CLIPA_ERR_ARG, and so is C >= 2^20. */
int clipa_zeroshot_ranks(const float* A, const float* W, const int32_t* labels, int64_t B, int64_t C, int64_t E, int64_t Lmax,
                         int64_t lda, int64_t ldw, int32_t* gt, int32_t* eq, int32_t* pred, void* stream);
/* Top-k similarity search (the `output.topk` of clipa_torch/training/zero_shot.py:47-50 and the top-k lists of
 * clipa_jax/evaluators/proj/image_text/image_text_retrieval.py:77-82) without the [Nq, Ng] matrix: Q [Nq, ldq] queries, G
 * [Ng, ldg] gallery rows (ldq, ldg >= E, multiples of 4), v_ij = fl(s * Q_i . G_j) by the arithmetic of clipa_retrieval_ranks
 * (one ascending-k fp32 chain; s = scale[0] read on the device, NULL = 1).  out_val f32 / out_idx int64 [Nq, k], 1 <= k <= 32:
 * the first k entries of row i, best first, under the strict total order
 *   (v, g) precedes (v', g') iff v > v', or v == v' and g < g',       g = index_base + j (0 <= index_base < 2^62).
 * `==` is IEEE equality: -0 and +0 tie, and a zero is reported as +0.  A NaN precedes every number (torch.topk's convention),
 * NaNs order among themselves by index and are reported as one quiet NaN: a poisoned row shows it in its first slot.  With
 * fewer than k entries the tail slots hold value -inf and index -1; they come after every real entry.  The order is strict, so
 * the result depends on the set of entries alone - not on tiles, splits, timing or shards - and is bit-reproducible; no float
 * atomics.
 * Shards: carry_val / carry_idx [Nq, k] (both or neither; same k; index -1 = empty slot, its value ignored) hold the lists of
 * earlier calls over other, disjoint index ranges; the output is the first k of (carry U this call's entries) and may alias
 * the carry.  The shards of a gallery in any sequence give bit for bit the lists of one call over the whole gallery.
 * Launches: the grid is (128-row query tiles) x splits, each split sweeping a contiguous range of the 128-row gallery tiles
 * into per-row lists in the workspace, then one wave per row merges the splits and the carry.  splits = 0 lets the entry choose
 * (min(gallery tiles, max(1, 512 / query tiles)): two workgroups for each of 256 CUs); any value in [1, gallery tiles] gives the
 * same output.  Workspace: clipa_topk_workspace(Nq, Ng, k, splits) bytes = splits * Nq * k * 8 (at least 16), O(Nq k) memory.
 * Nq == 0 returns CLIPA_OK without a launch.  Ng == 0 or E == 0 with Nq > 0 is valid (Q and G are then not read and may be
 * NULL): the output is the carry, or empty lists; E == 0 with Ng > 0 makes every value +0, so the indices run from index_base.
 * CLIPA_ERR_ARG before any launch: k outside [1, 32], negative sizes, Nq or Ng >= 2^31 - 128 (a larger gallery goes through
 * shards), 128 * ld * 4 >= 2^30, leading dimensions below E or not multiples of 4, null or not 16-byte aligned pointers, one
 * carry pointer without the other, index_base out of range, splits outside [0, max(1, gallery tiles)], query tiles * splits
 * >= 2^31, workspace too small. */
int64_t clipa_topk_workspace(int64_t Nq, int64_t Ng, int64_t k, int64_t splits);
int clipa_topk(const float* Q, const float* G, int64_t Nq, int64_t Ng, int64_t E, int64_t ldq, int64_t ldg, const float* scale,
               int64_t k, int64_t index_base, int64_t splits, const float* carry_val, const int64_t* carry_idx, float* out_val,
               int64_t* out_idx, void* workspace, int64_t workspace_bytes, void* stream);

/* AdamW over one flat tensor (training/main.py:318-326 torch.optim.AdamW + train.py:285-286 clamp is
 * done by the caller): p -= lr*(m_hat/(sqrt(v_hat)+eps) + wd*p). param/grad bf16 or f32; m, v f32. */
int clipa_adamw(void* param, const void* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int param_f32,
                int grad_f32, float lr, float beta1, float beta2, float eps, float weight_decay,
                int64_t step, float grad_scale, void* stream);
/* The same update over `count` tensors that share dtypes, hyper-parameters and step (one parameter group of
 * main.py:311-326): HOST arrays of device pointers / element counts; a few launches instead of one per tensor.
 * Fused optimizer tail (train.py:270-286): grad_scale_dev (optional DEVICE float, e.g. the clip coefficient of
 * clipa_clip_coef) multiplies every gradient; tensor `clamp_index` (-1: none) is clamped to [clamp_lo, clamp_hi]
 * after its update (logit_scale.clamp_(0, ln 100)). */
int clipa_adamw_multi(void* const* params, const void* const* grads, float* const* exp_avg,
                      float* const* exp_avg_sq, const int64_t* numel, int count, int param_f32, int grad_f32,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                      float grad_scale, const float* grad_scale_dev, int clamp_index, float clamp_lo, float clamp_hi,
                      void* stream);
/* torch.nn.utils.clip_grad_norm_ (train.py:270-277) without a host round trip: acc[0] += sum of squares of the listed
 * gradients (zero it first; call once per dtype bucket), then coef = min(1, max_norm / (sqrt(acc) + 1e-6)) and the
 * norm itself land in device memory for clipa_adamw_multi's grad_scale_dev.  `partials` is caller-provided scratch of at
 * least sum_i ceil(numel[i] / 4096) floats: block partials are summed in a fixed order (no float atomics - the coefficient is
 * bit-reproducible run to run). */
int clipa_grad_sqnorm_multi(const void* const* grads, const int64_t* numel, int count, int grad_f32, float* acc,
                            float* partials, int64_t partials_cap, void* stream);
int clipa_clip_coef(const float* acc, float max_norm, float* norm_out, float* coef_out, void* stream);
/* Sharded gradient exchange (replaces the ring all-reduce of the DDP wrapper, training/main.py:292-299):
 * out[i] = scale * sum over w < W of in[w*n + i] - the local sum of the W shard pieces a rank receives in the one-hop
 * all-to-all form of a reduce-scatter (scale = 1/W: DDP's gradient average).  bf16 or f32 in / out, fp32 sums in rank
 * order; n % 8 == 0. */
int clipa_reduce_shards(const void* in, void* out, int64_t n, int W, int in_f32, int out_f32, float scale, void* stream);
/* Image-tower fine-tuning (csrc/mixcut.hip, csrc/softce.hip).
 * Batch Mixup / CutMix IN PLACE on uint8 [B,3,S,S] in NCHW (nhwc = 0) or channels_last (nhwc = 1) memory - replaces the image
 * half of MixupAndCutmix, clipa_jax/transforms/mixup.py:141-201 with the box of transforms/random_erasing.py:25-61: sample b is
 * mixed with its mirror B-1-b (tf.reverse, mixup.py:179,199).  mode 0 mixup, lam f32 [B]: out_b = lam_b x_b + (1 - lam_b)
 * x_{B-1-b} per byte as d = a - b', t = lam d, v = t + b', out = (uint8)(int)(v + 0.5f) in fp32 without contraction (box
 * unused, may be NULL).  mode 1 cutmix, box int32 [B][4] = (y0, y1, x0, x1) half-open, inside the image: out_b = x_{B-1-b}
 * inside box_b and x_b outside (lam unused, may be NULL).  With odd B the middle sample is untouched.  Descriptors are validated
 * on the device first: a pair with lam outside [0, 1] or NaN, or with a box outside the image or y0 > y1 or x0 > x1, is left as
 * it was and counted in err_count (device int32, may be NULL).  S <= 4096, B <= 131070. */
int clipa_mixcut_u8(void* img, const float* lam, const int32_t* box, int64_t B, int64_t S, int nhwc, int mode, int32_t* err_count,
                    void* stream);
/* Soft-target cross-entropy in one pass - replaces softmax_xent, clipa_jax/losses/common.py:104-109, on the mixed and smoothed
 * labels of clipa_jax/transforms/mixup.py:203-211 without the [B, C] target matrix: logits f32 [B, ld], 2 <= C <= 32768 real
 * columns (columns >= C are never read), ld % 4 == 0; ya int32 [B], yb int32 [B] with lam f32 [B] or both NULL (lam = 1);
 *   t_c = (1 - smoothing) (lam [c = ya] + (1 - lam) [c = yb]) + smoothing / C;
 *   lse[i] = log sum_c exp z_ic, loss[i] = lse[i] - sum_c t_c z_ic, and where dlogits is given
 *   dlogits[i, c] = gscale (softmax(z_i)_c - t_c) as bf16 [B, ldd], ldd % 8 == 0, columns C .. ldd - 1 written as zero.
 * One wave per row, fixed summation order (csrc/softce.hip), no float atomics: bit-identical for every max_workgroups (0 = one
 * workgroup per four rows).  A label outside [0, C) or lam outside [0, 1] or NaN is counted in err_count (device int32, may be
 * NULL): that row's loss and lse are NaN, its gradient row zero.  The mean of the row losses is a clipa_sum_scale launch. */
int clipa_softce(const float* logits, int64_t B, int64_t C, int64_t ld, const int32_t* ya, const int32_t* yb, const float* lam,
                 float smoothing, float gscale, float* loss, float* lse, void* dlogits, int64_t ldd, int64_t max_workgroups,
                 int32_t* err_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
