/* libuenc_hip.so — C ABI of the MI355X (gfx950) kernels behind the unified-encoder hot path.
 *
 * Drop-in boundary.  The reference is a Python / Detectron2 plug-in whose only foreign-function
 * interface is the pybind11 module `MultiScaleDeformableAttention`
 * (model/modeling/pixel_decoder/ops/src/vision.cpp:18-21, ms_deform_attn.h:25-66).  Entry points
 * `uenc_msdeform_attn_{fwd,bwd}` replace exactly that pair with the same tensor contract.  Every other
 * entry point replaces a group of ATen calls that the reference issues from Python (cited per function);
 * the Python side (`uni-encoder-code_amd/uenc/kernels.py`, ctypes) binds all of them.
 *
 * Conventions
 *   - plain pointers and sizes only: device pointers are `void*` / typed pointers into HBM,
 *     sizes are element counts, strides ("ld*") are in elements; no framework types;
 *   - return 0 = launched, < 0 = invalid argument (shape / alignment / dtype; nothing was launched),
 *     > 0 = hipError_t from the launch;
 *   - the caller owns every buffer (inputs, outputs, scratch); the library allocates nothing, never
 *     synchronises, and launches on the given stream (`uenc_stream_t` = `hipStream_t`, passed as void*);
 *   - stateless and re-entrant, with one opt-in exception: the `uenc_prof_*` launch timers;
 *   - dtype tags: UENC_F32 = 0, UENC_BF16 = 1.  bf16 operands, fp32 accumulation everywhere.
 *   - gfx950 only.
 */
#ifndef UENC_H
#define UENC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UENC_F32 0
#define UENC_BF16 1

/* The launch stream.  A HIP stream handle is a pointer; C callers (ctypes, cgo, JNI) pass it as void*.  The library's own
 * sources define UENC_STREAM_T as hipStream_t before including this header, so that hipcc checks every definition in
 * the csrc .hip files against the declaration here (same ABI: one pointer). */
#ifndef UENC_STREAM_T
#define UENC_STREAM_T void*
#endif
typedef UENC_STREAM_T uenc_stream_t;

/* GEMM epilogues */
#define UENC_EPI_NONE 0       /* C = alpha * (A W^T + bias)                                   */
#define UENC_EPI_GELU 1       /* C = gelu(.) (erf form); optional aux_out <- pre-activation    */
#define UENC_EPI_RELU 2       /* C = relu(.)                                                   */
#define UENC_EPI_RESIDUAL 3   /* C = (.) + aux            aux fp32, may alias C                */
#define UENC_EPI_MUL_DGELU 4  /* C = (.) * gelu'(aux)     aux bf16 = saved pre-activation      */
#define UENC_EPI_MUL_DRELU 5  /* C = (.) * (aux > 0)      aux bf16 = saved ReLU output         */

int uenc_version(void);
const char* uenc_arch(void); /* "gfx950" */

/* ---- casts: fp32 master weights -> bf16 MFMA operands (replaces autocast-style .to(bf16)) ---------- */
int uenc_cast_f32_bf16(const float* src, void* dst, long n /* multiple of 8 */, uenc_stream_t stream);
/* Inverted dropout on a bf16 tensor of n elements (n % 8 == 0; in place allowed): out[i] = keep(i) ? in[i] / (1 - p) : 0 with
 * keep(i) = hash(seed, i) >= p * 2^32 (the index hash the attention kernels use for attention-probability dropout).  The mask is a
 * function of (seed, i): the backward calls the same entry on the gradient.  Replaces nn.Dropout between the deformable encoder
 * layer's kernels in training mode (reference pixel_decoder/msdeformattn.py:111-119, 121-142). */
int uenc_dropout_bf16(const void* in, void* out, long n, unsigned seed, float p, uenc_stream_t stream);
int uenc_cast_transpose_f32_bf16(const float* src /* [R][C] */, void* dst /* [C][R] bf16 */, int R, int C, uenc_stream_t stream);

/* batched cast: `table` = n device-resident descriptors {const float* src; bf16* dst; int rows, cols, transpose, tiles_c;
 * long tile_begin;} (40 bytes each; tiles_c = ceil(cols / 64), tile_begin = exclusive prefix sum of 64x64 tile counts);
 * dst is [rows][cols] or, if (transpose & 1), [cols][rows]; transpose >> 4, when non-zero, is the leading dimension of dst in elements
 * (several sources filling row / column blocks of one destination).  One launch refreshes every bf16 weight operand of a model. */
int uenc_cast_multi(const void* table, int n, long total_tiles, uenc_stream_t stream);

/* bilinear resize, align_corners = False, of NC fp32 planes (Hi, Wi) -> (Ho, Wo), Wo % 4 == 0: the final mask upsample
 * F.interpolate(mask_pred_results, size=..., mode="bilinear") of model/oneformer_model.py:255-263 (forward only). */
int uenc_upsample_bilinear(const float* in, float* out, long NC, int Hi, int Wi, int Ho, int Wo, uenc_stream_t stream);

/* attention mask of the masked-attention decoder: mask[r][oy][ox] = bilinear(logits[r], (Ho, Wo))[oy][ox] < 0 (1 = blocked),
 * rows that would be fully blocked are cleared (reference oneformer_transformer_decoder.py:497-505 and :454).
 * logits fp32 [rows][Hi][Wi]; mask u8 [rows][Ho][Wo]. */
int uenc_attn_mask(const float* logits, uint8_t* mask, long rows, int Hi, int Wi, int Ho, int Wo, uenc_stream_t stream);

/* ---- glue of the deformable encoder layer (pixel_decoder/ops/modules/ms_deform_attn.py:91-113) ---------------------
 * out = bf16(a + b), b repeating every `period` elements (n % period == 0, both % 4 == 0): query = src + pos. */
int uenc_add_cast_bf16(const float* a, const float* b, void* out, long n, long period, uenc_stream_t stream);
/* offaw (rows, ld) fp32 = [M][L][P][2] sampling offsets | [M][L*P] attention logits per row (row = image * Lq + query):
 * loc (rows, M, L, P, 2) = ref + off / (W_l, H_l), aw (rows, M, L*P) = softmax(logits).  ref (N|1, Lq, L, 2) fp32
 * (ref_per_image: 1 if it has a batch dimension), shapes (L, 2) int64 device.  L * P <= 16. */
int uenc_msda_prep_fwd(const float* offaw, long ld, const float* ref, int ref_per_image, const int64_t* shapes, float* loc,
                       float* aw, long rows, int Lq, int M, int L, int P, uenc_stream_t stream);
/* doffaw (rows, ld) bf16 <- d(loc), d(aw) and the saved softmax aw. */
int uenc_msda_prep_bwd(const float* dloc, const float* daw, const float* aw, const int64_t* shapes, void* doffaw, long ld,
                       long rows, int Lq, int M, int L, int P, uenc_stream_t stream);
/* out (nseg, 128, cols) fp32 = 128 partial column sums per segment (the caller adds them) of the bf16 matrix x16 over row
 * segments [seg_start[s], seg_start[s+1]) of every image (rows_per_image rows each): per-level sums for the level-embedding
 * gradient.  cols % 8 == 0. */
int uenc_segment_colsum(const void* x16, long ld, int cols, const int64_t* seg_start, int nseg, long rows_per_image, int images,
                        float* out, uenc_stream_t stream);

/* ---- FPN branch of the pixel decoder on token matrices (pixel_decoder/msdeformattn.py:283-304, :343-352) -----------
 * y = GroupNorm(x) [+ bilinear_resize(add_src, align_corners=False)] [ReLU] for x, y (B, HW, C) fp32|bf16 (torch.nn.GroupNorm
 * semantics over (HW x C/G) per image and group).  stats (B, G, 2) = (mean, rstd) is written for the backward; scratch:
 * uenc_groupnorm_tokens_scratch_bytes().  add_src: NULL or fp32 (B, Hs, Ws, C), then HW == H * W.  C % G == 0, (C/G) % 4 == 0,
 * 64 % (C/G) == 0, 256 % (C/4) == 0.  relu != 0 together with add_src != NULL returns UENC_EINVAL: the backward has no add_src
 * argument and recomputes the ReLU mask from xhat * gamma + beta alone, without the merged term, so the pair could only be
 * differentiated wrongly.  (The reference's ReLU follows the output convolution, never the merge.) */
long uenc_groupnorm_tokens_scratch_bytes(int B, int HW, int C, int G);
int uenc_groupnorm_tokens_fwd(const void* x, int x_dtype, const float* gamma, const float* beta, void* y, int y_dtype,
                              float* stats, void* scratch, const float* add_src, int Hs, int Ws, int H, int W, int B, int HW,
                              int C, int G, float eps, int relu, uenc_stream_t stream);
/* dx (B, HW, C) fp32|bf16; dgamma / dbeta (C) accumulated (may be NULL); relu != 0: the mask is recomputed from x. */
int uenc_groupnorm_tokens_bwd(const void* dy, int dy_dtype, const void* x, int x_dtype, const float* gamma, const float* beta,
                              const float* stats, void* dx, int dx_dtype, float* dgamma, float* dbeta, void* scratch, int B,
                              int HW, int C, int G, int relu, uenc_stream_t stream);
/* adjoint of the bilinear merge: dsrc (B, Hs, Ws, C) fp32 overwritten from dy (B, H, W, C) fp32|bf16, H >= Hs, W >= Ws. */
int uenc_upsample_bilinear_tokens_bwd(const void* dy, int dy_dtype, float* dsrc, int B, int H, int W, int Hs, int Ws, int C,
                                      uenc_stream_t stream);
/* Nearest-neighbour top-down merge of the plain FPN decoders (csrc/fpn_nearest.hip; reference pixel_decoder/fpn.py:151, :304):
 * out (B, H, W, C) = a (B, H, W, C) + prev (B, Hs, Ws, C)[nearest], every tensor fp32|bf16, the sum taken in fp32; source index
 * min((int)floorf(dst * ((float)Hs / H)), Hs - 1) as F.interpolate(mode="nearest").  C % 4 == 0; fp32 tensors 16-byte, bf16 8-byte
 * aligned.  Adjoint: dprev (B, Hs, Ws, C) fp32, every element written = the fp32 sum, in row-major order of the destination, of the
 * dy pixels whose forward index is that pixel (a gather, no atomics); any size ratio. */
int uenc_merge_nearest_tokens_fwd(const void* a, int a_dtype, const void* prev, int prev_dtype, void* out, int out_dtype, int B, int H, int W,
                                  int Hs, int Ws, int C, uenc_stream_t stream);
int uenc_merge_nearest_tokens_bwd(const void* dy, int dy_dtype, float* dprev, int B, int H, int W, int Hs, int Ws, int C,
                                  uenc_stream_t stream);
/* 3x3 / stride 1 / pad 1 convolution as a GEMM (bf16, C % 8 == 0): col (B*H*W, 9*C) with column (ky, kx, c) from
 * in (B, H, W, C), and the adjoint dx (B, H, W, C) from dcol (B*H*W, 9*C). */
int uenc_im2col3x3(const void* in, void* col, int B, int H, int W, int C, uenc_stream_t stream);
int uenc_col2im3x3(const void* dcol, void* dx, int B, int H, int W, int C, uenc_stream_t stream);
/* The same for the 3x3 stride-2 pad-1 convolutions of DiNAT's ConvTokenizer / ConvDownsampler (reference
 * model/modeling/backbone/dinat.py:17-45): col (B * ceil(H/2) * ceil(W/2), 9C) bf16 in (ky, kx, c) order; the adjoint gathers
 * dcol back to dx (B, H, W, C) fp32, every element written once.  C % 8 == 0. */
int uenc_im2col3x3_s2(const void* in, void* col, int B, int H, int W, int C, uenc_stream_t stream);
int uenc_col2im3x3_s2(const void* dcol, float* dx, int B, int H, int W, int C, uenc_stream_t stream);

/* ---- Linear layers ---------------------------------------------------------------------------------
 * C[m][n] = epi(alpha * (sum_k A[m][k] W[n][k] + bias[n])).  A fp32|bf16 [M][K] (lda), W bf16 [N][K] (ldw),
 * C fp32|bf16 [M][N] (ldc).  K % 8 == 0, N % 4 == 0, 16-byte aligned bases.  splitk > 1 or accumulate != 0
 * adds into fp32 C with atomics (EPI_NONE only).
 * Replaces nn.Linear / F.linear / 1x1 Conv2d / einsum("bqc,bchw->bqhw") of
 *   backbone/swin.py:35-41,138-170,335  pixel_decoder/ops/modules/ms_deform_attn.py:103-125
 *   pixel_decoder/msdeformattn.py:126-130,237,266,290  transformer_decoder/oneformer_transformer_decoder.py:183,498-500
 *   and nn.MultiheadAttention's in/out projections (transformer.py:252-253). */
int uenc_gemm_nt(const void* A, int a_dtype, long lda, const void* W, long ldw, void* C, int c_dtype, long ldc,
                 int M, int N, int K, const float* bias, int epilogue, const void* aux, long ldaux,
                 void* aux_out, long ldaux_out, float alpha, int splitk, int accumulate, uenc_stream_t stream);
/* The same on the large-tile kernel the caller names instead of the one the library's measured rules would pick (tile = 0: exactly
 * uenc_gemm_nt).  For tests and A/B measurements.  The tile replaces the choice only: where the shape is not one that kernel takes
 * (bf16 A, N >= 192, N % 8 == 0, K >= 128, K % 64 == 0 -- K % 32 == 0 for 128 x 256 --, at least 160 tiles of 256 x 256; no split-K /
 * accumulate on the 256 x 192 and 128 x 256 tiles) the call returns -1 and launches nothing. */
#define UENC_NT_TILE_256X256 256
#define UENC_NT_TILE_256X192 192
#define UENC_NT_TILE_128X256 128
int uenc_gemm_nt_tile(const void* A, int a_dtype, long lda, const void* W, long ldw, void* C, int c_dtype, long ldc,
                      int M, int N, int K, const float* bias, int epilogue, const void* aux, long ldaux,
                      void* aux_out, long ldaux_out, float alpha, int splitk, int accumulate, int tile, uenc_stream_t stream);
/* uenc_gemm_nt with alpha multiplied per SAMPLE: row m uses alpha * sample_scale[m / rows_per_sample] (sample_scale: device fp32).
 * Stochastic depth as an epilogue -- timm DropPath(x) = x * floor(keep + U) / keep per image (reference backbone/swin.py:8, 279, 289):
 * the residual-branch GEMM runs over all images at once, a dropped image's rows come out as the residual alone.  Stored results only. */
int uenc_gemm_nt_scaled(const void* A, int a_dtype, long lda, const void* W, long ldw, void* C, int c_dtype, long ldc,
                        int M, int N, int K, const float* bias, int epilogue, const void* aux, long ldaux,
                        void* aux_out, long ldaux_out, float alpha, const float* sample_scale, int rows_per_sample, uenc_stream_t stream);
/* Linear -> residual add -> LayerNorm with the LayerNorm inside the GEMM's epilogue (pixel_decoder/msdeformattn.py:111-142 at d_model 256,
 * backbone/swin.py:262-295 at C = 192): C (M, N) fp32, ldc == N, receives the pre-norm sum h = A W^T + bias + residual (the LayerNorm
 * backward reads it), y32 / y16 (either may be NULL) the normalised rows as fp32 / bf16, stats (M, 2) = (mean, rstd) (may be NULL).
 * The row must fit one column tile of an LDS-staged kernel: N <= 256, N % 8 == 0, bf16 A, K % 64 == 0, M large enough for the tiled kernels;
 * returns -1 (nothing launched) otherwise: run uenc_gemm_nt + uenc_layernorm_fwd then (same numbers up to fp32 summation order). */
int uenc_gemm_nt_ln(const void* A, int a_dtype, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias,
                    const void* residual, long ldres, const float* gamma, const float* beta, float eps, float* y32, void* y16, float* stats,
                    uenc_stream_t stream);
/* Split-K with STORED partial sums (no atomics): split s of `splitk` writes its fp32 partial product to P + s * part_stride
 * (row stride ldp); the caller sums the slices.  splitk must equal uenc_gemm_nt_splits(K, requested) (the number of non-empty
 * k-ranges after rounding to 64).  Replaces the reference's torch.einsum("bqc,bchw->bqhw") backward w.r.t. the mask embedding
 * (model/modeling/transformer_decoder/oneformer_transformer_decoder.py:500) for all prediction heads at once. */
int uenc_gemm_nt_splits(int K, int splitk);
int uenc_gemm_nt_partials(const void* A, int a_dtype, long lda, const void* W, long ldw, float* P, long ldp, long part_stride,
                          int M, int N, int K, float alpha, int splitk, uenc_stream_t stream);

/* `batch` problems of one shape in one launch (problem b: A + b*bsA, W + b*bsW -> C + b*bsC, element strides, byte
 * offsets multiples of 16); no bias / epilogue; split-K and accumulate as above. */
int uenc_gemm_nt_batched(const void* A, int a_dtype, long lda, long bsA, const void* W, long ldw, long bsW, void* C, int c_dtype,
                         long ldc, long bsC, int batch, int M, int N, int K, float alpha, int splitk, int accumulate, uenc_stream_t stream);

/* weight / bias gradient of the same Linear:  dW[n][k] += sum_m dY[m][n] X[m][k];  db[n] += sum_m dY[m][n]
 * (db may be NULL).  dY, X fp32|bf16 row-major; dW, db fp32, accumulated (atomics).  N % 8 == K % 8 == 0.
 * splitm <= 0 lets the library choose the split of the token dimension.  Replaces autograd's
 * mm / sum backward of every Linear above. */
int uenc_gemm_tn(const void* dY, int dy_dtype, long ldy, const void* X, int x_dtype, long ldx, float* dW, long ldw,
                 float* db, int M, int N, int K, int splitm, uenc_stream_t stream);
/* The same on the LDS-DMA kernel with the output tile the caller names (tile = 256 or 128; 0: exactly uenc_gemm_tn).  For tests.
 * Returns -1 and launches nothing unless both operands are bf16, M % 64 == 0 and M >= 2048. */
int uenc_gemm_tn_tile(const void* dY, int dy_dtype, long ldy, const void* X, int x_dtype, long ldx, float* dW, long ldw,
                      float* db, int M, int N, int K, int splitm, int tile, uenc_stream_t stream);
/* dW += alpha * dY^T X, db += alpha * column sums: the weight gradient of a residual branch whose output was scaled by alpha
 * (stochastic depth, timm DropPath at reference backbone/swin.py:279, 289; the branch's dropped images are left out of M). */
int uenc_gemm_tn_scaled(const void* dY, int dy_dtype, long ldy, const void* X, int x_dtype, long ldx, float* dW, long ldw,
                        float* db, int M, int N, int K, int splitm, float alpha, uenc_stream_t stream);

/* Grouped weight gradients: one launch for many (dY, X, dW, db) problems of the form above (bf16 operands only).
 * table: n descriptors in DEVICE memory, 96 bytes each:
 *   { const void* dY, *X; float* dW, *db; long ldy, ldx, ldw; int M, N, K, tiles_k, mlen, nsplit, item_begin, store; float alpha; int zero; }
 * alpha multiplies the problem's sums (0 is read as 1).
 * M % 64 == 0; mlen (tokens per split, % 64 == 0) * nsplit >= M; tiles_k = ceil(K / tile); item_begin = exclusive prefix
 * sum of ceil(N / tile) * tiles_k * nsplit; total_items = the full sum.  tile = 256 or 128.  Accumulates into dW / db
 * (atomic adds), or, for a descriptor with store != 0 and nsplit == 1, overwrites them with plain stores.
 * flops = 2 * sum(M N K), used by uenc_prof_* only. */
int uenc_gemm_tn_grouped(const void* table, int n, int total_items, int tile, double flops, uenc_stream_t stream);
/* The same for the register-staged kernel (any M, fp32|bf16 operands, 128 x 128 tiles): descriptors of 96 bytes
 *   { const void* dY, *X; float* dW, *db; long ldy, ldx, ldw; int M, N, K, dy_f32, x_f32, tiles_k, mlen, nsplit, item_begin; float alpha; }   (alpha: as above)
 * tiles_k = ceil(K / 128), mlen % 64 == 0, item_begin = exclusive prefix sum of ceil(N / 128) * tiles_k * nsplit. */
int uenc_gemm_tn_grouped_small(const void* table, int n, int total_items, double flops, uenc_stream_t stream);

/* ---- LayerNorm over the last dimension (C % 4 == 0, C <= 6144) --------------------------------------
 * y = LN(x + res) * gamma + beta; optional h_out <- x + res (fp32); optional stats <- (mean, rstd) per row.
 * Replaces nn.LayerNorm and the preceding residual add of swin.py:247,293,334,492,673,
 * msdeformattn.py:128-129,136-137, transformer.py:268-297, oneformer_transformer_decoder.py:66-67,126-127,184-185,496. */
int uenc_layernorm_fwd(const void* x, int x_dtype, const void* res, int res_dtype, float* h_out, const float* gamma,
                       const float* beta, void* y, int y_dtype, float* stats, long M, int C, float eps, void* y16,
                       uenc_stream_t stream);
/* dx = LN'(dy) [+ dres];  dgamma / dbeta accumulated (both NULL to skip).
 * y16 / dx16 (may be NULL): a bf16 copy of y / dx written in the same pass -- the operand the next GEMM reads, so that an
 * fp32 stream needs no separate cast kernel.  part_ws (may be NULL): scratch of 2048 * 2 * C floats; with it the
 * workgroups' dgamma / dbeta partials are stored and summed by a second small kernel instead of added atomically. */
int uenc_layernorm_bwd(const void* dy, int dy_dtype, const void* h, int h_dtype, const float* stats, const float* gamma,
                       const float* dres, void* dx, int dx_dtype, float* dgamma, float* dbeta, long M, int C, void* dx16,
                       float* part_ws, int defer_param_sums, uenc_stream_t stream);
/* Deferred parameter sums.  With part_ws and defer_param_sums != 0 the block partials of dgamma / dbeta stay in part_ws -- [nblk][2][C]
 * floats, nblk = uenc_layernorm_bwd_blocks(M, C) (0: the pass adds its few block sums itself and nothing is deferred) -- and NO reduction is
 * launched; the caller keeps part_ws untouched and later sums the partials of many passes in ONE launch:
 *   table: n descriptors in DEVICE memory, 40 bytes each { const float* part; float* dgamma; float* dbeta; int nblk, C, group_begin, pad; },
 *   group_begin = exclusive prefix sum of ceil(2C / 64), total_groups = the full sum; dgamma / dbeta are accumulated.
 * (A training step leaves ~70 such reductions of a few MB each: 10 us launches for 2 us of work.) */
int uenc_layernorm_bwd_blocks(long M, int C);
int uenc_ln_param_grouped(const void* table, int n, int total_groups, uenc_stream_t stream);
/* PatchMerging's pad-to-even + 2x2 strided gather + concat (order (0,0), (1,0), (0,1), (1,1)) + LayerNorm(4C) as one pass
 * (reference model/modeling/backbone/swin.py:311-334; the 4C -> 2C reduction GEMM follows): x (B, H, W, C) fp32 ->
 * y (B * ceil(H/2) * ceil(W/2), 4C) bf16, stats (rows, 2).  Backward: dy (rows, 4C) bf16 | fp32 -> dx (B, H, W, C) fp32 written
 * completely; dgamma / dbeta (4C) accumulated; part_ws as for uenc_layernorm_bwd. */
int uenc_patch_merge_ln_fwd(const float* x, const float* gamma, const float* beta, void* y, float* stats, int B, int H, int W,
                            int C, float eps, uenc_stream_t stream);
int uenc_patch_merge_ln_bwd(const void* dy, int dy_dtype, const float* x, const float* stats, const float* gamma, float* dx,
                            float* dgamma, float* dbeta, float* part_ws, int B, int H, int W, int C, int defer_param_sums,
                            uenc_stream_t stream);          /* rows M = B * ceil(H/2) * ceil(W/2), width 4C for uenc_layernorm_bwd_blocks */

/* ---- shifted-window attention (head_dim 32, window <= 12) ---------------------------------------------
 * Replaces F.pad -> torch.roll -> window_partition -> WindowAttention core -> window_reverse -> roll -> crop,
 * backbone/swin.py:250-289 around :131-171, shift mask of :414-440.
 * qkv (B,H,W,3C) bf16 = qkv Linear output of the real tokens; qkv_bias (3C) bf16 (value of padding slots);
 * bias_q / bias_k: expanded relative-position bias from uenc_relpos_expand; out (B,H,W,C) bf16. */
int uenc_window_attn_np(int ws); /* padded tokens per window = 16 * ceil(ws*ws / 16) */
int uenc_relpos_expand(const float* table /* ((2ws-1)^2, nH) */, float* bias_q /* (nH,NP,NP) [h][q][key] */,
                       float* bias_k /* (nH,NP,NP) [h][key][q] */, int nH, int ws, uenc_stream_t stream);
/* Grouped form: n descriptors in device memory (8-byte aligned), 40 bytes each
 * { const float* table; float* bias_q; float* bias_k (NULL: not written); int nH, ws, NP, blk_begin; } with NP =
 * uenc_window_attn_np(ws) and blk_begin = exclusive prefix sum of ceil(nH*NP*NP / 2048); total_blocks = the full sum.  One
 * launch refreshes the expanded biases of every window-attention module after an optimizer step (the host keeps them keyed by
 * the table's version: uenc.ops.ParamCache.relpos).  (The window-attention kernels do not read bias_k any more: it may alias
 * bias_q in their calls.) */
int uenc_relpos_expand_grouped(const void* table, int n, int total_blocks, uenc_stream_t stream);
/* lse (B,H,W,nH) fp32 or NULL: the softmax row statistics max + log2(sum) of every real token and head (scores in log2 units), written
 * by the forward; given back to uenc_window_attn_bwd, the 12 x 12 backward computes the probabilities from them instead of repeating
 * the maximum / sum passes (other window sizes, and lse == NULL, recompute). */
int uenc_window_attn_fwd(const void* qkv, const void* qkv_bias, const float* bias_q, void* out, float* lse, int B, int H, int W,
                         int C, int nH, int ws, int shift, float scale, uenc_stream_t stream);
/* dqkv (B,H,W,3C) bf16 written.  dS_ws: scratch of uenc_window_attn_bwd_ws_floats() floats (dense per-workgroup sums of
 * dS, overwritten).  The two parameter gradients are ACCUMULATED (+=, float atomics) straight into the caller's buffers, i.e.
 * into attn.relative_position_bias_table.grad and attn.qkv.bias.grad: dtable ((2ws-1)^2, nH) fp32 in the parameter's own
 * layout; dbias_pad (3C) fp32 = the q | k | v slice of the qkv.bias gradient that flows through padding slots (the zero rows
 * F.pad appends after norm1, swin.py:254, whose q/k/v equal the bias). */
long uenc_window_attn_bwd_ws_floats(int B, int H, int W, int nH, int ws);
int uenc_window_attn_bwd(const void* qkv, const void* qkv_bias, const float* bias_q, const float* bias_k,
                         const void* o_saved, const float* lse /* of uenc_window_attn_fwd, or NULL */, const void* d_out, void* dqkv,
                         float* dS_ws, float* dtable, float* dbias_pad,
                         int B, int H, int W, int C, int nH, int ws, int shift, float scale, int defer_dtable, uenc_stream_t stream);
/* defer_dtable != 0: dqkv and dbias_pad as above, but the relative-position-table gradient is NOT reduced: dS_ws keeps the dense partials
 * [nH][G][ntiles][NP * 16] (G = uenc_window_attn_bwd_groups(...), ntiles = NP / 16) and the caller, keeping dS_ws untouched, reduces the
 * partials of many passes in one launch: table = n descriptors in DEVICE memory, 40 bytes each
 * { const float* wsd; float* dtab; int G, nH, ws, ntiles, blk_begin, pad; }, blk_begin = exclusive prefix sum of nH * ntiles. */
int uenc_window_attn_bwd_groups(int B, int H, int W, int nH, int ws);
int uenc_window_attn_dtable_grouped(const void* table, int n, int total_blocks, uenc_stream_t stream);

/* ---- multi-scale deformable attention: the reference's native op ---------------------------------------
 * ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step)
 *   (ops/src/ms_deform_attn.h:25-45, kernel ops/src/cuda/ms_deform_im2col_cuda.cuh:242-304):
 * value (B,S,M,D) fp32|bf16, shapes (L,2) int64 (H,W), level_start (L) int64, loc (B,Lq,M,L,P,2) fp32,
 * attn (B,Lq,M,L,P) fp32 -> out (B,Lq,M*D) fp32|bf16.  D in {16,32,64}.  im2col_step is not needed:
 * one launch covers the batch. */
int uenc_msdeform_attn_fwd(const void* value, int v_dtype, const int64_t* shapes, const int64_t* level_start,
                           const float* loc, const float* attn, void* out, int out_dtype, int B, int S, int M, int D,
                           int L, int Lq, int P, uenc_stream_t stream);
/* The same forward for the geometry of the deformable ENCODER (ops/modules/ms_deform_attn.py called from
 * pixel_decoder/msdeformattn.py:115-121: the queries are the pixels of the L maps, Lq == S, level-major), with the value pixels a
 * neighbourhood of queries samples staged once per workgroup in LDS instead of gathered tap by tap from L2.  Same arguments and
 * result plus shapes_host, the HOST copy of `shapes`.  Needs D == 32, bf16 value, L <= 4, L * P <= 16, Lq == S == sum(H_l * W_l);
 * returns -1 (nothing launched) otherwise -- call uenc_msdeform_attn_fwd then.  Any sampling locations are legal: a level whose
 * sampled box does not fit the LDS budget is gathered from memory as in the general kernel. */
int uenc_msdeform_attn_fwd_tiled(const void* value, int v_dtype, const int64_t* shapes, const int64_t* level_start,
                                 const float* loc, const float* attn, void* out, int out_dtype, int B, int S, int M, int D,
                                 int L, int Lq, int P, const int64_t* shapes_host, uenc_stream_t stream);
/* ms_deform_attn_backward (ms_deform_attn.h:47-66, cuh:306-408): grad_value fp32 accumulated (caller zeroes,
 * as the reference's at::zeros_like), grad_loc / grad_attn overwritten.  shapes_host: optional HOST copy of `shapes`,
 * workspace: optional device scratch of uenc_msdeform_attn_bwd_workspace_bytes() bytes (both may be NULL).  With them
 * (D == 32, L <= 4, L*P <= 16) the grad_value contributions are binned per block of value pixels and summed on chip
 * instead of being sent to memory one float atomic per tap and channel.  Same result either way. */
int uenc_msdeform_attn_bwd(const void* value, int v_dtype, const int64_t* shapes, const int64_t* level_start,
                           const float* loc, const float* attn, const void* grad_out, int go_dtype, float* grad_value,
                           float* grad_loc, float* grad_attn, int B, int S, int M, int D, int L, int Lq, int P,
                           const int64_t* shapes_host, void* workspace, long workspace_bytes, uenc_stream_t stream);
long uenc_msdeform_attn_bwd_workspace_bytes(const int64_t* shapes_host, int B, int M, int D, int L, int Lq, int P);
/* Fused form of the same op for callers that own the two projection Linears around it (ops/modules/ms_deform_attn.py:99-125): instead
 * of sampling locations and attention weights the kernels take the projection row they are derived from,
 *   offaw (B * Lq, ld) fp32 = [M][L][P][2] sampling offsets | [M][L * P] attention logits   (sampling_offsets | attention_weights Linear outputs),
 * the reference points ref (B | 1, Lq, L, 2) fp32 (ref_per_image: 1 if ref has a batch dimension) and the level shapes:
 * loc = ref + off / (W_l, H_l), attn = softmax over the L * P logits, both computed inside the kernels.  The backward writes
 * d(offaw) (B * Lq, ld_doffaw) bf16 (all 3 M L P columns) and accumulates grad_value (caller zeroes) -- grad_loc / grad_attn never exist.
 * L * P <= 16, D == 32, ld even; the backward needs shapes_host + workspace (uenc_msdeform_attn_bwd_workspace_bytes() > 0) and
 * returns -1 otherwise.  Same sums as uenc_msda_prep_fwd + uenc_msdeform_attn_fwd (and the backward pair). */
int uenc_msdeform_attn_fused_fwd(const void* value, int v_dtype, const int64_t* shapes, const int64_t* level_start, const float* offaw,
                                 long ld, const float* ref, int ref_per_image, void* out, int out_dtype, int B, int S, int M, int D,
                                 int L, int Lq, int P, uenc_stream_t stream);
/* The fused forward for the encoder's geometry with the value tiles in LDS (uenc_msdeform_attn_fwd_tiled with the locations / weights derived
 * inside the kernel): P == 4, ld % 4 == 0, 16-byte aligned offaw / out; -1 (nothing launched) when not eligible. */
int uenc_msdeform_attn_fused_fwd_tiled(const void* value, int v_dtype, const int64_t* shapes, const int64_t* level_start, const float* offaw,
                                       long ld, const float* ref, int ref_per_image, void* out, int out_dtype, int B, int S, int M, int D,
                                       int L, int Lq, int P, const int64_t* shapes_host, uenc_stream_t stream);
int uenc_msdeform_attn_fused_bwd(const void* value, int v_dtype, const int64_t* shapes, const int64_t* level_start, const float* offaw,
                                 long ld, const float* ref, int ref_per_image, const void* grad_out, int go_dtype, float* grad_value,
                                 void* doffaw, long ld_doffaw, int B, int S, int M, int D, int L, int Lq, int P, const int64_t* shapes_host,
                                 void* workspace, long workspace_bytes, uenc_stream_t stream);

/* ---- decoder multi-head attention core (head_dim 32) --------------------------------------------------------
 * softmax(scale * q k^T [blocked where mask != 0]) v for every nn.MultiheadAttention of the transformer decoder
 * (transformer_decoder/oneformer_transformer_decoder.py:63-67,122-127 with the mask of :504-511; transformer.py:268-297).
 * q (B,Lq,*) / k, v (B,S,*) bf16 with heads interleaved in the row (head h at columns 32h..32h+31); *_bs / *_rs are
 * batch / row strides in elements (multiples of 8).  mask (B,Lq,mask_rs) bytes, shared by all heads, mask_rs a multiple
 * of 4 and >= S, or NULL.  out (B,Lq,*) bf16; lse (B,H,Lq) fp32 log2-domain log-sum-exp (needed by the backward).
 * workspace: uenc_mha_fwd_workspace_floats(...) floats (split-KV partials); NULL when that is 0.
 * dropout_p in [0, 1), seed: dropout on the attention probabilities AFTER the softmax normalisation, as
 * nn.MultiheadAttention(dropout=p) applies it in training mode (transformer.py:249-250, 0.1 in the class transformer): element
 * (b, h, q, key) is kept iff hash(seed, ((b H + h) Lq + q) S + key) >= p 2^32 and scaled by 1 / (1 - p); the backward regenerates
 * the mask from the same (p, seed).  0 = off (inference, and every masked-attention layer: their rate is 0.0, :326-344). */
long uenc_mha_fwd_workspace_floats(int B, int H, int Lq, int S);
int uenc_mha_fwd(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs,
                 long v_rs, const unsigned char* mask, long mask_rs, void* out, long o_bs, long o_rs, float* lse,
                 float* workspace, int B, int H, int Lq, int S, float scale, float dropout_p, unsigned seed, uenc_stream_t stream);
/* dq (B,Lq,*) fp32 ACCUMULATED (caller zeroes); dk, dv (B,S,*) bf16 overwritten for every key and head.
 * Lq <= 960 without a mask and <= 640 with one: the dK / dV kernel keeps all queries in LDS, slices = ceil(Lq / 160),
 * slices * 160 * 136 + 16384 (+ 64 * (slices * 160 + 4) with a mask) <= 160 KB.  A longer Lq returns UENC_EINVAL before anything is
 * launched (dq included). */
int uenc_mha_bwd(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs,
                 long v_rs, const unsigned char* mask, long mask_rs, const void* out, long o_bs, long o_rs,
                 const float* lse, const void* dout, long do_bs, long do_rs, float* dq, long dq_bs, long dq_rs, void* dk,
                 long dk_bs, long dk_rs, void* dv, long dv_bs, long dv_rs, int B, int H, int Lq, int S, float scale,
                 float dropout_p, unsigned seed, uenc_stream_t stream);

/* ---- neighbourhood attention 2-D (DiNAT backbone) -------------------------------------------------------------
 * What natten.NeighborhoodAttention2D computes between its qkv and proj Linear layers (reference call site
 * model/modeling/backbone/dinat.py:14, 77-79, 94; NATTEN 0.14.4's natten2dqkrpb + softmax + natten2dav -- the wheel is not
 * part of the reference tree: parity unpinned, restated in oracle/dinat_ref.py).  head_dim is 32.
 * qkv (B, H, W, 3, nH, 32) bf16 = the qkv Linear's output as is; rpb (nH, 2K-1, 2K-1) fp32 or NULL; out (B, H, W, nH, 32)
 * bf16; lse (B, nH, H, W) fp32 natural-log log-sum-exp (NULL for inference).  K odd in 3..13; H, W >= K * dilation (the
 * caller zero-pads smaller inputs first, as NATTEN does); scale = head_dim^-0.5 applied to q.k. */
int uenc_na2d_fwd(const void* qkv, const float* rpb, void* out, float* lse, int B, int H, int W, int nH, int K, int dilation,
                  float scale, uenc_stream_t stream);
/* dqkv (B, H, W, 3, nH, 32) bf16 overwritten completely; drpb (nH, 2K-1, 2K-1) fp32 ACCUMULATED (may be NULL);
 * delta_ws: B * nH * H * W floats of scratch. */
int uenc_na2d_bwd(const void* qkv, const float* rpb, const void* out, const void* dout, const float* lse, void* dqkv, float* drpb,
                  float* delta_ws, int B, int H, int W, int nH, int K, int dilation, float scale, uenc_stream_t stream);

/* ---- segmentation post-processing fused with the mask upsample (inference) ---------------------------------------
 * The reference upsamples the (Q, h, w) mask logits to the padded input size (model/oneformer_model.py:255-263), crops the
 * padding (detectron2 sem_seg_postprocess, :277-279) and then runs semantic_inference (:367-371) / panoptic_inference
 * (:373-434) on the 1.25 GB-per-image result.  These entry points interpolate on the fly from the low-resolution logits
 * (bilinear, align_corners = False to (Hp, Wp); output extent (Ho, Wo) <= (Hp, Wp) = the crop); all tensors fp32 / int32,
 * one image per call.
 *   semantic:        sem (C, Ho, Wo) = sum_q class_prob[q, c] * sigmoid(up(mask_logits[q])); class_prob (Q, Cp), Cp % 32 == 0
 *   panoptic_stats:  ids (Ho, Wo) = argmax_q score[q] * sigmoid(up(m_q)) over queries with score > 0 (first maximum wins);
 *                    counts (3, Q), zeroed by the caller: |ids == q|, |sigmoid(up(m_q)) >= 0.5|, |both| -- what the reference
 *                    reads back with three .item() syncs per query (:399-408)
 *   panoptic_label:  seg (Ho, Wo) = segid[ids] where that query's sigmoid >= 0.5, else 0 (:420-425); segid (Q), 0 = dropped */
int uenc_postproc_semantic(const float* mask_logits, const float* class_prob, float* sem, int Q, int C, int Cp, int hl, int wl,
                           int Hp, int Wp, int Ho, int Wo, uenc_stream_t stream);
int uenc_postproc_panoptic_stats(const float* mask_logits, const float* score, int* ids, int* counts, int Q, int hl, int wl, int Hp,
                                 int Wp, int Ho, int Wo, uenc_stream_t stream);
int uenc_postproc_panoptic_label(const float* mask_logits, const int* ids, const int* segid, int* seg, int Q, int hl, int wl, int Hp,
                                 int Wp, int Ho, int Wo, uenc_stream_t stream);

/* ---- fp32 "exact" arithmetic mode (csrc/exact.hip; UENC_EXACT=1 / uenc.ops.set_exact) -----------------------------------
 * The reference computes in fp32 end to end (AMP off, configs/cityscapes/swin/unified_encoder_cityscapes.yaml:27-28; the pixel
 * decoder forces fp32, pixel_decoder/msdeformattn.py:336,343).  These entry points run the contractions of the path on fp32
 * operands with fp32 accumulation (v_mfma_f32_16x16x4_f32 for the GEMMs, VALU for the three attention cores), so that a
 * deviation from the reference can be split into bf16 rounding (the product's mode) and everything else (must be ~1e-5).
 * A verification mode: same call sites, same epilogues, no performance claim.
 *   gemm_nt_f32:  C = epi(alpha * (A W^T + bias)), all fp32, K % 4 == 0, lda / ldw % 4 == 0; aux / aux_out fp32 (the
 *                 GELU pre-activation, ReLU output or residual of the UENC_EPI_* epilogues); accumulate: C += (EPI_NONE only)
 *   gemm_tn_f32:  dW (N, K) += dY^T X, db (N) += column sums of dY (db may be NULL); dY (M, N), X (M, K) fp32, N, K % 4 == 0
 *   window_attn_f32_{fwd,bwd}: qkv (B, H, W, 3C) fp32, qkv_bias (3C), table ((2ws-1)^2, nH) = relative_position_bias_table,
 *                 out / dout (B, H, W, C); same pad / shift / mask semantics as uenc_window_attn_* (model/modeling/backbone/
 *                 swin.py:250-289, :131-171, :414-440) and the same window domain: ws 1 .. 12, 0 <= shift < ws, C == 32 nH; anything
 *                 else is UENC_EINVAL before a launch.  bwd: dqkv written, dtable and dbias_pad (3C) accumulated (atomics)
 *   mha_f32_{fwd,bwd}: the decoder's nn.MultiheadAttention cores, tensor contract of uenc_mha_* with fp32 tensors; lse (B, nH, Lq);
 *                 bwd: dq written, dk / dv (zeroed by the caller) accumulated, delta (B, nH, Lq) scratch
 *   na2d_f32_{fwd,bwd}: DiNAT's neighbourhood attention, tensor contract and limits of uenc_na2d_* with fp32 tensors: qkv
 *                 (B, H, W, 3, nH, 32), out / dout (B, H, W, nH, 32), rpb (nH, 2K-1, 2K-1) or NULL, lse (B, nH, H, W) (NULL
 *                 allowed in the forward); bwd: dqkv written completely, drpb accumulated (atomics; may be NULL) */
int uenc_gemm_nt_f32(const float* A, long lda, const float* W, long ldw, float* C, long ldc, int M, int N, int K, const float* bias,
                     int epilogue, const float* aux, long ldaux, float* aux_out, long ldaux_out, float alpha, int accumulate, uenc_stream_t stream);
int uenc_gemm_tn_f32(const float* dY, long ldy, const float* X, long ldx, float* dW, long ldw, float* db, int M, int N, int K, uenc_stream_t stream);
int uenc_window_attn_f32_fwd(const float* qkv, const float* qkv_bias, const float* table, float* out, int B, int H, int W, int C, int nH,
                             int ws, int shift, float scale, uenc_stream_t stream);
int uenc_window_attn_f32_bwd(const float* qkv, const float* qkv_bias, const float* table, const float* dout, float* dqkv, float* dtable,
                             float* dbias_pad, int B, int H, int W, int C, int nH, int ws, int shift, float scale, uenc_stream_t stream);
int uenc_mha_f32_fwd(const float* q, long qs0, long qs1, const float* k, long ks0, long ks1, const float* v, long vs0, long vs1,
                     const uint8_t* mask, long mask_row_stride, float* out, long os0, long os1, float* lse, int B, int nH, int Lq, int S,
                     float scale, float dropout_p, unsigned seed, uenc_stream_t stream);
int uenc_mha_f32_bwd(const float* q, long qs0, long qs1, const float* k, long ks0, long ks1, const float* v, long vs0, long vs1,
                     const uint8_t* mask, long mask_row_stride, const float* out, long os0, long os1, const float* lse, const float* dout,
                     long gos0, long gos1, float* dq, long dqs0, long dqs1, float* dk, long dks0, long dks1, float* dv, long dvs0, long dvs1,
                     float* delta, int B, int nH, int Lq, int S, float scale, float dropout_p, unsigned seed, uenc_stream_t stream);
int uenc_na2d_f32_fwd(const float* qkv, const float* rpb, float* out, float* lse, int B, int H, int W, int nH, int K, int dilation,
                      float scale, uenc_stream_t stream);
int uenc_na2d_f32_bwd(const float* qkv, const float* rpb, const float* out, const float* dout, const float* lse, float* dqkv, float* drpb,
                      int B, int H, int W, int nH, int K, int dilation, float scale, uenc_stream_t stream);

/* ---- device-side per-step randomness (capturable training step, uenc/graphs.py) ---------------------------------------------- */
/* state = {64-bit base seed, 64-bit step counter} in device memory.  advance != 0: step += 1 first (by the kernel: a replayed graph
 * needs no host input).  Then, with key = mix(base, step) (the attn_keep hash):
 *   scales[s * n_samples + b] = keep ? 1 / keep_prob[s] : 0,  keep = hash(key, 2^41 | (s n_samples + b)) >= (1 - keep_prob[s]) 2^32
 *   seeds[j] = hash(key, 2^40 | j)
 * for the n_branch DropPath branch slots and n_seed dropout seed slots.  Pure functions of (base, step, slot, sample). */
int uenc_step_rng_advance(unsigned long long* state, const float* keep_prob, int n_branch, int n_samples, float* scales, int n_seed,
                          unsigned* seeds, int advance, uenc_stream_t stream);
/* Inverted dropout of n elements (dtype UENC_F32 / UENC_BF16, any n, in place allowed) with the seed read from seeds[slot] on the device:
 * the keep-mask of uenc_dropout_bf16, bit-identical to it for bf16 and the same seed. */
int uenc_dropout_sp(const void* in, void* out, long n, int dtype, const unsigned* seeds, int slot, float p, uenc_stream_t stream);
/* out[r][:C] = bf16(in[r][:C] * sample_scale[r / rows_per_sample]) for r < M (bf16 rows, C % 8 == 0, 16-byte aligned rows): the
 * DropPath-scaled gradient a branch's weight-gradient GEMM reads when the multipliers live on the device. */
int uenc_scale_rows_bf16(const void* in, long ld_in, void* out, long ld_out, long M, int C, const float* sample_scale, long rows_per_sample,
                         uenc_stream_t stream);
/* hipMemcpyAsync of `bytes` from pinned host memory to the device on `stream` (the descriptor uploads of a captured step). */
int uenc_upload(void* dst, const void* src, long bytes, uenc_stream_t stream);
/* uenc_mha_fwd / uenc_mha_bwd with the dropout seed read from seeds[slot] on the device (bit-identical for the same seed). */
int uenc_mha_fwd_sp(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs,
                    long v_rs, const unsigned char* mask, long mask_rs, void* out, long o_bs, long o_rs, float* lse,
                    float* workspace, int B, int H, int Lq, int S, float scale, float dropout_p, const unsigned* seeds, int slot,
                    uenc_stream_t stream);
int uenc_mha_bwd_sp(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs,
                    long v_rs, const unsigned char* mask, long mask_rs, const void* out, long o_bs, long o_rs,
                    const float* lse, const void* dout, long do_bs, long do_rs, float* dq, long dq_bs, long dq_rs, void* dk,
                    long dk_bs, long dk_rs, void* dv, long dv_bs, long dv_rs, int B, int H, int Lq, int S, float scale,
                    float dropout_p, const unsigned* seeds, int slot, uenc_stream_t stream);

/* ---- query-tiled attention core (csrc/attn_tiled.hip): a whole feature map attending to itself (the DETR encoder of
 * TransformerEncoderPixelDecoder, reference modeling/pixel_decoder/fpn.py:155-232 on transformer.py:161-234) ---------------------------
 * Tensor contract of uenc_mha_fwd / uenc_mha_bwd without mask and workspace, head_dim 32, any Lq >= 1 and S >= 1 (the query count is
 * bounded by the grid alone: ceil(Lq / 64) * B * H and ceil(S / 64) * B * H below 2^31).  q, k, v, out, dout: bf16, row / batch
 * strides multiples of 8 elements and 16-byte aligned pointers (out in the forward: multiples of 4, 8-byte aligned); lse (B, H, Lq)
 * fp32, log2 domain.  Dropout as uenc_mha_fwd: element index ((b H + h) Lq + q) S + key.
 * Backward: dq (B, Lq, *) fp32 WRITTEN (strides multiples of 4, 16-byte aligned), dk, dv (B, S, *) bf16 written (strides multiples
 * of 4, 8-byte aligned).  Two kernels (dQ per query tile, dK / dV per key tile), no atomics, nothing to zero: the same input gives
 * the same bits.  uenc_attn_tiled_tile(0) = queries per workgroup, (1) = keys per LDS block / per dK-dV workgroup. */
int uenc_attn_tiled_tile(int which);
int uenc_attn_tiled_fwd(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs,
                        long v_rs, void* out, long o_bs, long o_rs, float* lse, int B, int H, int Lq, int S, float scale,
                        float dropout_p, unsigned seed, uenc_stream_t stream);
int uenc_attn_tiled_bwd(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs,
                        long v_rs, const void* out, long o_bs, long o_rs, const float* lse, const void* dout, long do_bs,
                        long do_rs, float* dq, long dq_bs, long dq_rs, void* dk, long dk_bs, long dk_rs, void* dv, long dv_bs,
                        long dv_rs, int B, int H, int Lq, int S, float scale, float dropout_p, unsigned seed,
                        uenc_stream_t stream);
int uenc_attn_tiled_fwd_sp(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs,
                           long v_rs, void* out, long o_bs, long o_rs, float* lse, int B, int H, int Lq, int S, float scale,
                           float dropout_p, const unsigned* seeds, int slot, uenc_stream_t stream);
int uenc_attn_tiled_bwd_sp(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs,
                           long v_rs, const void* out, long o_bs, long o_rs, const float* lse, const void* dout, long do_bs,
                           long do_rs, float* dq, long dq_bs, long dq_rs, void* dk, long dk_bs, long dk_rs, void* dv,
                           long dv_bs, long dv_rs, int B, int H, int Lq, int S, float scale, float dropout_p,
                           const unsigned* seeds, int slot, uenc_stream_t stream);

/* ---- fused AdamW with full-model gradient clipping (csrc/optim.hip; replaces the reference's optimizer wrapper, tools/calc_throughput.py:
 * torch.nan_to_num on every gradient, clip_grad_norm_ over all of them, torch.optim.AdamW) ------------------------------------------------
 * `table` = n device-resident segment descriptors, one per parameter tensor (56 bytes each):
 *   {float* param; const float* grad; float* exp_avg; float* exp_avg_sq; long n; long tile_begin; int group; int pad;}
 * tile_begin = exclusive prefix sum of ceil((n + a) / 4096) with a = ((uintptr_t)param / 4) % 4 (tiles start on 16-byte boundaries of the
 * parameter; gradient and moments may sit at any 4-byte offset); total_tiles = the sum.  All tensors fp32, dense.
 * `state` = 32-byte device block, 16-byte aligned: {long long step; double norm; float clip_coef, inv_bc1, inv_sqrt_bc2, pad;}.  The caller
 * initialises it to {steps taken, 0, 1, 0, 0, 0}; nothing a launch computes depends on a value the host read back.
 * Gradients are sanitised as they are read (NaN -> 0, +inf -> 1e5, -inf -> -1e5) and never written. */
/* step += 1 and the bias corrections 1 / (1 - beta1^step), 1 / sqrt(1 - beta2^step) of the new step: first launch of an optimizer step. */
int uenc_optim_advance(void* state, double beta1, double beta2, uenc_stream_t stream);
/* state.norm = sqrt(sum of squares of all sanitised gradients), state.clip_coef = min(1, max_norm / (norm + 1e-6)).  Two stages without
 * atomics (per-workgroup partial sums into `partials`, n_partials >= min(total_tiles, 2048) doubles, then one workgroup in a fixed order):
 * bit-identical from run to run.  Skipped when clipping is off (clip_coef stays 1). */
int uenc_optim_grad_sqnorm(const void* table, int n, long total_tiles, double* partials, int n_partials, void* state, float max_norm,
                           uenc_stream_t stream);
/* torch.optim.AdamW's update (decoupled decay, no amsgrad, no maximize) of every segment with gradient = sanitised * state.clip_coef, at
 * step count state.step.  `groups` = n_groups x {float lr, weight_decay, 1 - lr * weight_decay, unused} (16-byte aligned device array)
 * indexed by the segment's group. */
int uenc_optim_adamw_step(const void* table, int n, long total_tiles, const float* groups, int n_groups, const void* state, double beta1,
                          double beta2, double eps, uenc_stream_t stream);

/* ---- bipartite matching (csrc/matcher.hip; reference model/modeling/matcher.py) ----------------------------------------------------------
 * A batch of independent problems, problem = one prediction head of one image.  `probs` is a HOST array of n_prob descriptors which the
 * call copies into its kernel arguments (no device table; a stream capture records the pointers they hold by value).  Nothing is read
 * back and nothing synchronises. */
/* The cost matrix of HungarianMatcher.memory_efficient_forward (matcher.py:126-171) for every problem.  Descriptor (48 bytes):
 *   {const float* logits (Q, C1); const float* masks (Q, h, w); const float* points (P, 2) x, y in [0, 1]; const unsigned char* gt (T, Hg, Wg)
 *    0 / 1; const int64* labels (T); int T; int pad;}
 * Prediction and target are both sampled bilinearly at the P points (point_sample = grid_sample at 2 p - 1, align_corners = False, zero
 * padding, matcher.py:143-155); cost_mask = (softplus(-x).t + softplus(x).(1 - t)) / P (matcher.py:61-85), cost_dice = 1 - (2 sigmoid(x).t
 * + 1) / (sum sigmoid(x) + sum t + 1) (matcher.py:38-53), cost_class = -softmax(logits)[:, label] (matcher.py:128-134);
 * C = w_mask cost_mask + w_class cost_class + w_dice cost_dice (matcher.py:166-170), NaN entries become `nan_fill` (100: matcher.py:33-34; a caller
 * that wants to see them passes NaN; a label outside [0, C1) counts as NaN).  fp32 throughout, partial sums added in a fixed order: the same input gives the same bits.
 * `cost` = (n_prob, Q, Tmax) fp32, row stride Tmax; columns >= a problem's T are written as ZERO.  Limits: 1 <= Q, Tmax <= 256,
 * 0 <= T <= Tmax.  `workspace` = uenc_match_cost_workspace_floats(...) floats, 16-byte aligned; the sampled values stay in LDS. */
long uenc_match_cost_workspace_floats(int n_prob, int Q, int Tmax, int P);
int uenc_match_cost(const void* probs, int n_prob, int Q, int C1, int h, int w, int Hg, int Wg, int P, int Tmax, float w_class, float w_mask,
                    float w_dice, float nan_fill, float* workspace, long workspace_floats, float* cost, uenc_stream_t stream);
/* scipy.optimize.linear_sum_assignment (matcher.py:36, 173) of every problem's Q x T matrix: shortest augmenting paths with duals in
 * double, one workgroup per problem.  Descriptor (32 bytes): {const float* cost (Q, ld); int64* row_ind; int64* col_ind; int T; int ld;}.
 * Writes min(Q, T) pairs in scipy's convention (row_ind ascending, col_ind the matched column); T = 0 writes nothing.  A NaN entry is
 * read as 100 and entries are clamped to +-1e30, so the search always terminates.  Limits: 1 <= Q <= 256, 0 <= T <= 256, ld >= T. */
int uenc_lsap_solve(const void* probs, int n_prob, int Q, uenc_stream_t stream);

/* ---- set criterion (csrc/criterion.hip; uenc.modeling.criterion.SetCriterion) ---------------------------------------------------------------
 * Point-sampled mask and dice losses of the matched pairs and the weighted class loss, ALL prediction heads per call, fp32, no float
 * atomics: the same input gives the same bits.  A pair is one matched (query, target) of one image of one head; a head's pairs run over the
 * images in order, within an image in the matcher's order, N = sum_b min(Q, T_b) per head, and row r = head * N + n of every buffer is
 * pair n of that head.  row_ind / col_ind are the matcher's flat DEVICE index buffers (n_heads * N int64 each: the query and the target of
 * every pair); a pair whose indices are out of range is inert (zero losses, no gradient).  `desc` is a HOST block of 1024 bytes which the
 * call copies into its kernel arguments (a stream capture records the pointers by value):
 *   {struct {const float* masks (bs, Q, h, w); const float* logits (bs, Q, C1);} head[16];
 *    struct {const unsigned char* gt (T, Hg, Wg) 0 / 1; const int64* labels (T); int T; int pair0;} img[32];}
 * with pair0 = the sum of min(Q, T) over the images before.  Limits: n_heads <= 16, bs <= 32, Q, T <= 256, maps up to 16384 x 16384,
 * P, M <= 2^21.  Sampling is grid_sample at 2 p - 1 (bilinear, align_corners = False, zero padding), as in uenc_match_cost. */
/* out (n_heads * N, M): the predicted logit map of every pair at its M points, points = (n_heads * N, M, 2) x, y in [0, 1]. */
int uenc_crit_point_logits(const void* desc, int n_heads, int bs, int Q, int h, int w, int N, int M, const long long* row_ind,
                           const float* points, float* out, uenc_stream_t stream);
/* Per pair, x_p = logit map and t_p = target mask at point p of points (n_heads * N, P, 2):
 *   loss[r] = {ce_n = (1 / P) sum_p bce_with_logits(x_p, t_p), dice_n = 1 - (2 sum s t + 1) / (sum s + sum t + 1)}, s = sigmoid(x);
 *   sums[r] = {sum s t, sum s, sum t}.
 * With unit and keys given (both or neither): unit (n_heads * N, P, 2) = {d ce_n / d x_p, d dice_n / d x_p} and keys (n_heads * N, P, 4)
 * int32, 16-byte aligned = the cell y * w + x of the point's four taps (nw, ne, sw, se), h * w for a tap outside the map. */
int uenc_crit_mask_loss_fwd(const void* desc, int n_heads, int bs, int Q, int h, int w, int Hg, int Wg, int N, int P, const long long* row_ind,
                            const long long* col_ind, const float* points, float* loss, float* sums, float* unit, int* keys,
                            uenc_stream_t stream);
/* gmasks (n_heads, bs, Q, h, w), ZERO-FILLED by the caller: the gradient of sum_head (gce[head] sum_n ce_n + gdice[head] sum_n dice_n) *
 * inv_num_masks to every head's mask logits.  sorted_keys / order (n_heads * N, 4 P) are a STABLE ascending sort of each row of `keys`
 * and its permutation (int64); gce / gdice are n_heads device floats.  The lane at the head of each run of equal keys adds the run in
 * sorted order and writes its cell once.  The queries of one image's pairs must be distinct, as those of an assignment are. */
int uenc_crit_mask_loss_bwd(const void* desc, int n_heads, int bs, int Q, int h, int w, int N, int P, const long long* row_ind,
                            const float* points, const float* unit, const int* sorted_keys, const long long* order, const float* gce,
                            const float* gdice, float inv_num_masks, float* gmasks, uenc_stream_t stream);
/* Per head: target class of row (b, q) = labels[col] of the image's pair whose query is q, else C1 - 1 (no object); weight 1, eos_coef for
 * no object; loss[head] = sum w nll / sum w (F.cross_entropy with weights) and grad (n_heads, bs * Q, C1) = w (softmax - onehot) / sum w.
 * rows = 2 * n_heads * bs * Q floats of workspace.  N may be 0 (no targets at all).  A label outside [0, C1) takes its row out of the loss. */
int uenc_crit_class_loss(const void* desc, int n_heads, int bs, int Q, int C1, int N, const long long* row_ind, const long long* col_ind,
                         float eos_coef, float* rows, float* loss, float* grad, uenc_stream_t stream);

/* ---- MonodepthLoss hot path (csrc/monodepth.hip; reference model/modeling/monodepth_loss.py:427-517, 671-680, 734-777) ---------------------
 * fp32, dense tensors, S <= 4 scales (scale s is (H >> s) x (W >> s); H and W divisible by 2^(S-1)), NF <= 2 source frames, no float atomics:
 * the same input gives the same bits.  `desc` is a HOST block of 67 pointers which the call copies into its kernel arguments (a stream
 * capture records them by value), index = scale * NF + frame where two are given:
 *   const float* disp[4] (B, 1, h, w); cflow[8] (B, 3, h, w); mask[8] (B, 1, h, w); T (NF, B, 4, 4); K (B, 4, 4); invK (B, 4, 4);
 *   src (NF, B, 3, H, W);
 *   float* color (S, NF, B, 3, H, W); sample (S, NF, B, H, W, 2); sample_ego; sample_cmp (as sample); depth (S, B, 1, H, W);
 *   residual[8] (B, 3, H, W);
 *   const float* gcolor (as color); gres[8] (as residual, NULL = zero);
 *   float* gdisp[4]; gcflow[8]; gmask[8] (as their inputs); gT (NF, B, 4, 4).
 * mode 0: rigid (sample = K T depth invK pix); 1: complete flow only (sample = K (X + flow)); 2: complete flow with the motion mask
 * (sample = K T (X + (flow - ego) mask)); modes 1 and 2 also write sample_ego, sample_cmp and residual = flow - ego at full resolution.
 * Per pixel: disp upsampled bilinearly (align_corners = False), depth = 1 / (0.01 + 9.99 disp), projection divided by z + 1e-7 and
 * normalised by (W - 1, H - 1), colour sampled with border padding and align_corners = True. */
int uenc_view_synth_fwd(const void* desc, int S, int NF, int B, int H, int W, int mode, uenc_stream_t stream);
/* Gradients of (gcolor, gres) to disp, cam_T_cam, complete flow and motion mask; every output element is written.  Two launches: per
 * full-resolution pixel into `workspace` (with per-block partial sums for cam_T_cam), then one gather per low-resolution pixel over its
 * bounded footprint and the partials added in a fixed order.  `workspace` = uenc_view_synth_workspace_floats(...) floats. */
long uenc_view_synth_workspace_floats(int S, int NF, int B, int H, int W);
int uenc_view_synth_bwd(const void* desc, int S, int NF, int B, int H, int W, int mode, float* workspace, long workspace_floats,
                        uenc_stream_t stream);
/* Per pixel and candidate 0.85 mean_c SSIM + 0.15 mean_c L1 against `target` (B, 3, H, W); SSIM = clamp((1 - ssim) / 2, 0, 1) over 3x3
 * means of the reflection-padded images, C1 = 1e-4, C2 = 9e-4.  Candidates: the NF warped frames color[s][f]; with automask = 1 the NF
 * source frames src (NF, B, 3, H, W) come first, each plus noise (S, B, NF, H, W) * 1e-5.  argmin (S, B, H, W) = index of the smallest
 * (the first on a tie), p_photo[s] = mean of the minimum over B * H * W (block partials in `workspace`, added in a fixed order). */
long uenc_photo_loss_workspace_floats(int S, int B, int H, int W);
int uenc_photo_loss_fwd(const float* color, const float* target, const float* src, const float* noise, int S, int NF, int B, int H, int W,
                        int automask, float* workspace, long workspace_floats, unsigned char* argmin, float* p_photo, uenc_stream_t stream);
/* grad_color (as color) = d(sum_s grad_p_photo[s] p_photo[s]) / d(color): through the selected candidate only, zero elsewhere. */
int uenc_photo_loss_bwd(const float* color, const float* target, const unsigned char* argmin, const float* grad_p_photo, int S, int NF, int B,
                        int H, int W, int automask, float* grad_color, uenc_stream_t stream);

/* ---- ConvNeXt block front end (csrc/dwconv.hip; reference model/modeling/backbone/convnext.py:32-33, 43-45) ------------------------------
 * 7x7 depthwise convolution (stride 1, zero padding 3) on a channels-last fp32 map, fused with the LayerNorm over channels that follows:
 *   y = dwconv7x7(x) + b,  h = LN_C(y) * gamma + beta.   x, y (B, H, W, C) fp32; w (C, 1, 7, 7) fp32; b (C) or NULL; h fp32 | bf16
 * (h_dtype); stats (B*H*W, 2) = (mean, rstd).  All arithmetic fp32.  C % 8 == 0, C <= 6144, B <= 65535; any H, W >= 1 (maps smaller than
 * the filter included); x, y, stats 16-byte aligned.  One launch: 8 x 8 pixel tiles, channels in slabs of 32 through a 25 KB LDS halo. */
int uenc_dwconv7_ln_fwd(const float* x, const float* w, const float* b, const float* gamma, const float* beta, float* y, void* h, int h_dtype,
                        float* stats, int B, int H, int W, int C, float eps, uenc_stream_t stream);
/* dy = LN'(dh) per pixel from the saved y / stats (dgamma, dbeta, part_ws, defer_param_sums exactly as for uenc_layernorm_bwd, rows
 * M = B*H*W), then dx = dwconv7x7^T(dy) [+ dout]: correlation with the flipped filter, same padding.  dh fp32 | bf16; dout NULL or the
 * (B, H, W, C) fp32 gradient arriving on the block's skip path; dy, dx (B, H, W, C) fp32, every element written, dy != dx.  dy is the
 * operand of uenc_dwconv7_bwd_weight.  Two launches. */
int uenc_dwconv7_ln_bwd_data(const void* dh, int dh_dtype, const float* y, const float* stats, const float* gamma, const float* w,
                             const float* dout, float* dy, float* dx, float* dgamma, float* dbeta, float* part_ws, int defer_param_sums,
                             int B, int H, int W, int C, uenc_stream_t stream);
/* dw[c][ky][kx] += sum_{b,y,x} dy[b][y][x][c] * x[b][y+ky-3][x+kx-3][c], db[c] += sum dy (db may be NULL).  No atomics: per-workgroup
 * partials are stored to `workspace` (uenc_dwconv7_bwd_weight_workspace_bytes(), 16-byte aligned) and added in a fixed order, so the
 * same inputs give the same bits. */
long uenc_dwconv7_bwd_weight_workspace_bytes(int B, int H, int W, int C);
int uenc_dwconv7_bwd_weight(const float* dy, const float* x, float* dw, float* db, void* workspace, long workspace_bytes, int B, int H, int W,
                            int C, uenc_stream_t stream);
/* Layer scale folded into a Linear (convnext.py:48-50: gamma * (W2 g + b2) run as W2' = gamma (.) W2 row-wise, b2' = gamma (.) b2).
 * From the folded layer's gradients dW2' (N, K), db2' (N, may be NULL):
 *   gW2 += gamma (.) dW2',  gb2 += gamma (.) db2',  ggamma[n] += sum_k dW2'[n][k] W2[n][k] + db2'[n] b2[n].
 * gW2 / gb2 / ggamma may each be NULL (frozen parameter); b2 NULL = no bias.  Fixed summation order. */
int uenc_layer_scale_grads(const float* dw2p, const float* db2p, const float* w2, const float* b2, const float* gamma, float* gw2, float* gb2,
                           float* ggamma, int N, int K, uenc_stream_t stream);

/* ---- ResNet backbone (csrc/resnet.hip): stem patch gather, max pooling, BatchNorm + residual + ReLU ----------------------
 * All maps channels-last, C % 8 == 0, 16-byte aligned; every dtype argument is UENC_F32 or UENC_BF16.  No atomics: per-channel
 * reductions store one partial per row slab to `workspace` (uenc_bn_workspace_floats(M, C) floats) and a second launch adds the
 * slabs in a fixed order, so the same inputs give the same bits.  Nothing is read back to the host.
 *
 * Patch matrix of a 7x7 stride-2 padding-3 convolution on x (B, 3, H, W) fp32 NCHW: col (B * Ho * Wo, 152), Ho = (H - 1) / 2 + 1,
 * column (ky * 7 + kx) * 3 + c, columns 147..151 zero.  Any H, W >= 1. */
int uenc_stem7x7_s2_patches(const float* x, void* col, int col_dtype, int B, int H, int W, uenc_stream_t stream);
/* max_pool2d(x, 3, 2, 1) on x (B, H, W, C) -> y (B, Ho, Wo, C) of the same dtype; padding counts as -inf.  idx (B, Ho, Wo, C) bytes:
 * the selected tap ky * 3 + kx, the first maximum in scan order (ATen's choice on ties).  The backward is a gather: every dx
 * element (all written) adds the dy of the at most 4 windows whose idx names it, in fp32. */
int uenc_maxpool3x3_s2_fwd(const void* x, void* y, void* idx, int dtype, int B, int H, int W, int C, uenc_stream_t stream);
int uenc_maxpool3x3_s2_bwd(const void* dy, const void* idx, void* dx, int dtype, int B, int H, int W, int C, uenc_stream_t stream);
long uenc_bn_workspace_floats(long M, int C);
/* mean, var (C) fp32 = per-channel mean and biased variance over the M > 1 rows of x (M, C): Welford per thread, Chan merges across
 * threads and slabs.  The second launch also updates running_mean / running_var (either may be NULL) with `momentum` and the
 * unbiased variance, and adds 1 to num_batches_tracked[0] (int64, may be NULL). */
int uenc_bn_stats(const void* x, int x_dtype, long M, int C, float* mean, float* var, float* running_mean, float* running_var,
                  long long* num_batches_tracked, float momentum, float* workspace, long workspace_floats, uenc_stream_t stream);
/* y = act(x * s[c] + t[c] (+ res)),  s = gamma / sqrt(var + eps),  t = beta - mean * s;  act = ReLU (relu != 0) or identity.
 * mean / var are the batch statistics (train) or the running ones (eval, frozen); gamma / beta NULL = 1 / 0; res NULL = none. */
int uenc_bn_act_fwd(const void* x, int x_dtype, const float* mean, const float* var, const float* gamma, const float* beta, const void* res,
                    int res_dtype, void* y, int y_dtype, long M, int C, float eps, int relu, uenc_stream_t stream);
/* With g = dy masked by y > 0 (relu != 0; y is the saved output) and xhat = (x - mean) / sqrt(var + eps):
 * reduce: sums (2, C) = (sum g, sum g * xhat) over the rows; dbeta += sums[0], dgamma += sums[1] where not NULL.
 * apply:  dx = gamma / sqrt(var + eps) * (g - sums[0] / M - xhat * sums[1] / M) (train != 0) or g * gamma / sqrt(var + eps) (eval,
 *         frozen: x and sums unused);  dres (may be NULL) = g, the gradient of the residual branch. */
int uenc_bn_act_bwd_reduce(const void* dy, int dy_dtype, const void* y, int y_dtype, const void* x, int x_dtype, const float* mean,
                           const float* var, long M, int C, float eps, int relu, float* sums, float* dgamma, float* dbeta, float* workspace,
                           long workspace_floats, uenc_stream_t stream);
int uenc_bn_act_bwd_apply(const void* dy, int dy_dtype, const void* y, int y_dtype, const void* x, int x_dtype, const float* mean,
                          const float* var, const float* gamma, const float* sums, void* dx, int dx_dtype, void* dres, int dres_dtype, long M,
                          int C, float eps, int relu, int train, uenc_stream_t stream);

/* ---- training targets from a panoptic id map (csrc/targets.hip; uenc.modeling.targets.build_targets) -----------------------------------------
 * One padded batch: pan (B, H, W) int32 segment ids; sizes (B, 2) = each image's own (h, w) <= (H, W), pixels outside it belong to no
 * segment whatever pan holds there; the segment table is one row of UENC_TARGETS_MAX_SEGMENTS entries per image, seg_ids (B, 256) int32
 * with n_seg (B) of them in use.  Ids are any int32 > 0 (an entry <= 0 matches nothing; of two equal ids the lower row is the pixel's row);
 * an id of the map that the table does not list has no row.  All pointers are DEVICE memory, all tables int32; B <= 65535 and
 * H * W < 2^31 - 4096.  Values that index memory (n_seg, sizes, slot, plane0, T) are clamped or made inert on the device, never trusted.
 * Each call is one launch, whatever n_seg is; no float arithmetic, the same input gives the same bits. */
#define UENC_TARGETS_MAX_SEGMENTS 256
/* area (B, 256) int32, ZERO-FILLED by the caller: area[b, r] += the number of pixels of image b, inside its own size, whose row is r
 * (counted in LDS; one integer atomic add per workgroup and row). */
int uenc_targets_area(const int* pan, const int* sizes, const int* seg_ids, const int* n_seg, int* area, int B, int H, int W,
                      uenc_stream_t stream);
/* slot (B, 256): the target plane of a row inside its image, or -1 (several rows may share a plane); cls (B, 256): the class a row writes
 * into the label map, or < 0; plane0 (B), T (B): image b owns planes plane0[b] .. plane0[b] + T[b] - 1 of masks (total_planes, H, W)
 * uint8, T[b] <= 256 (an image whose planes do not lie inside [0, total_planes) gets none; a slot outside [0, T[b]) counts as -1).
 *   masks[plane0[b] + t, y, x] = 1 where the pixel's row has slot t, else 0
 *   sem_seg[b, y, x] (int64)   = cls of the pixel's row; ignore_label where there is no row, where cls < 0, and in the padding
 * Every byte of sem_seg and of the planes the images own is written exactly once (nothing needs zeroing), with 16-byte stores when
 * H * W % 16 == 0 and pan, masks and sem_seg are 16-byte aligned. */
int uenc_targets_write(const int* pan, const int* sizes, const int* seg_ids, const int* n_seg, const int* slot, const int* cls,
                       const int* plane0, const int* T, long long ignore_label, unsigned char* masks, long long* sem_seg, int B, int H, int W,
                       int total_planes, uenc_stream_t stream);

/* ---- evaluation statistics on the device (csrc/evalstats.hip; uenc.evaluation SemSegEvaluator / PanopticEvaluator) ----------------------------
 * The same padded batch as the targets kernels: maps (B, H, W) int32, sizes (B, 2) = each image's own (h, w), pixels outside it are never
 * counted; B <= 65535, H * W < 2^31 - 4096; all pointers DEVICE memory, naturally aligned (16-byte loads are used when H * W % 4 == 0 and
 * the maps are 16-byte aligned).  Integer atomics only: the same input gives the same bits.  max_blocks: workgroups per image, 0 = as many
 * as the image has chunks of 4096 pixels (at most 512); fewer make a workgroup take several chunks. */
#define UENC_EVAL_MAX_CLASSES 1024
#define UENC_EVAL_PQ_DIM 258 /* UENC_TARGETS_MAX_SEGMENTS + 2 */
/* conf ((N + 1) x (N + 1)) int64, N = num_classes <= 1024: conf[p, g] += 1 per pixel.  C >= 1: pred is the scores (B, C, H, W) fp32 and
 * p the argmax over the C planes (lowest index on a tie; the first NaN wins as in torch.argmax); C == 0: pred is a label map (B, H, W)
 * int32.  p outside [0, N) counts in row N; g equal to ignore_label or outside [0, N) counts in column N. */
int uenc_eval_confusion(const void* pred, const int* gt, const int* sizes, long long* conf, int B, int C, int H, int W, int num_classes,
                        int ignore_label, int max_blocks, uenc_stream_t stream);
/* inter (B, 258, 258) int32, ZERO-FILLED by the caller: inter[b, r, c] += 1 per pixel, r from the pixel's ground-truth id and c from its
 * predicted id: 0 for id 0 (VOID), 1 + the id's row of gt_ids / pred_ids (B, 256; n_gt / n_pred (B) in use, rules as for seg_ids above),
 * n + 1 for an id that has no row ("unknown").  Rows above n_gt + 1 and columns above n_pred + 1 stay zero. */
int uenc_eval_pq_intersect(const int* pred, const int* gt, const int* sizes, const int* gt_ids, const int* n_gt, const int* pred_ids,
                           const int* n_pred, int* inter, int B, int H, int W, int max_blocks, uenc_stream_t stream);
/* panopticapi's pq_compute_single_core on inter, one workgroup per image; gt_cat, gt_crowd, pred_cat (B, 256) int32, K categories <= 1024.
 * Areas are the row / column sums.  A pair of real segments with inter > 0, the same category and a non-crowd ground truth matches when
 * 2 * inter > union = area_pred + area_gt - inter - inter[VOID, pred].  Every byte of the outputs is written:
 *   rec (B, 256, 4)  per ground-truth row: matched row of pred_ids or -1, inter, union (0, 0 without a match), category (-1 above n_gt)
 *   fn (B, K)        unmatched non-crowd ground-truth rows with area > 0, per category
 *   fp (B, K)        unmatched predicted rows unless 2 * (inter[VOID, pred] + their pixels over crowds of their category) > area_pred
 *   unknown (B)      pixels whose predicted id has no row
 * A category outside [0, K) is counted nowhere. */
int uenc_eval_pq_match(const int* inter, const int* n_gt, const int* n_pred, const int* gt_cat, const int* gt_crowd, const int* pred_cat,
                       int* rec, int* fp, int* fn, int* unknown, int B, int K, uenc_stream_t stream);

/* ---- depth decoder in training: the non-GEMM passes of TransDSSL (csrc/depth_head.hip) ----------------------------------------------------
 * Channels-last maps, operands fp32 | bf16 by their dtype tag, arithmetic in fp32, every pointer 16-byte aligned.  No float atomics:
 * each backward is a gather in a fixed order, two calls give the same bits. */
/* y (B, 2H, 2W, C) = bilinear resize of x (B, H, W, C) with align_corners=True, C % 8 == 0: source = o * ((H - 1) / (2H - 1)) with the
 * scale an fp32 division, i0 = floor, i1 = min(i0 + 1, H - 1) (F.interpolate's arithmetic); H == 1 or W == 1 copies along that axis. */
int uenc_upsample2x_ac_fwd(const void* x, int x_dtype, void* y, int y_dtype, int B, int H, int W, int C, uenc_stream_t stream);
/* dx (B, H, W, C), every element written = the adjoint applied to dy (B, 2H, 2W, C): each input cell gathers the outputs whose taps,
 * recomputed with the forward's own expression, touch it (row-major order of the outputs). */
int uenc_upsample2x_ac_bwd(const void* dy, int dy_dtype, void* dx, int dx_dtype, int B, int H, int W, int C, uenc_stream_t stream);
/* Per row of C channels (C % 8 == 0, C <= 2048): res = a + b, g = res * softmax_c(z) (row maximum subtracted).  res and g share out_dtype. */
int uenc_softmax_gate_fwd(const void* a, int a_dtype, const void* b, int b_dtype, const void* z, int z_dtype, void* res, void* g,
                          int out_dtype, long P, int C, uenc_stream_t stream);
/* att = softmax_c(z) recomputed;  d_res = dg * att + d_res_in (d_res_in NULL = 0),  d_z = att * (dg * res - sum_c(dg * res * att)).
 * d_res is the gradient of a and of b alike; d_res and d_z share out_dtype. */
int uenc_softmax_gate_bwd(const void* dg, int dg_dtype, const void* d_res_in, int d_res_in_dtype, const void* z, int z_dtype,
                          const void* res, int res_dtype, void* d_res, void* d_z, int out_dtype, long P, int C, uenc_stream_t stream);
/* disp (P) fp32 = sum_k softmax(z)_k * grid_k for z (P, D), grid (D) fp32; D % 8 == 0, D <= 64. */
int uenc_soft_att_depth_fwd(const void* z, int z_dtype, const float* grid, float* disp, long P, int D, uenc_stream_t stream);
/* dz_k = p_k * (grid_k - disp) * ddisp with p and disp recomputed from z; ddisp (P) fp32. */
int uenc_soft_att_depth_bwd(const float* ddisp, const void* z, int z_dtype, const float* grid, void* dz, int dz_dtype, long P, int D,
                            uenc_stream_t stream);

/* ---- training-time augmentation of one sample (csrc/augment.hip; uenc/train_data.py apply_plans) -------------------------------------------
 * The plan is the host's: the source (in_h, in_w) is resized to (rs_h, rs_w), the window (x0, y0, cw, ch) of the resized image is kept,
 * flipped horizontally when flip == 1, and padded (or cropped) at the right and bottom to (out_h, out_w).  Only the window is computed.
 * All pointers are DEVICE memory; int tables 4-byte aligned; integers only except the HSV -> BGR stage (float32, single rounded
 * operations: the same bits as the host's numpy expression).  No atomics, nothing is read back. */
#define UENC_AUG_TILE_W 64
#define UENC_AUG_TILE_H 16
#define UENC_AUG_MAX_TAPS 7
#define UENC_AUG_COLOUR_SAT 1            /* the saturation stage runs (HSV round trip, value table 2 on S) */
#define UENC_AUG_COLOUR_HUE 2            /* the hue stage runs (HSV round trip, H = (H + hue) mod 180) */
#define UENC_AUG_COLOUR_CONTRAST_FIRST 4 /* contrast before saturation and hue, else after them */
#define UENC_AUG_COLOUR_RGB 8            /* the frames are RGB (else BGR) */
#define UENC_AUG_COLOUR_TAB_INTS 704     /* 3 x 256 bytes of value tables (brightness, contrast, saturation), sdiv[256], hdiv[256] */
/* 1 when a 64 x 16 output tile of this resize fits the kernel's LDS (<= 165 source pixels x 40 source rows, kx, ky <= 7 taps), else 0. */
int uenc_augment_tile_fits(int in_h, int in_w, int rs_h, int rs_w, int kx, int ky);
/* dst (F, 3, out_h, out_w) uint8, every byte written, from F frames (in_h, in_w, 3) uint8, frame_stride bytes apart: PIL's BILINEAR
 * resize restricted to the window, then the SSD colour stages, flip, pad with pad_value.
 * col_tab: for each of the cw window columns the first source column, the tap count (<= kx) and kx 22-bit fixed-point coefficients,
 * laid out as first[cw], count[cw], coeff[cw][kx]; row_tab alike for the ch window rows with ky.  A pass computes
 * clip(((1 << 21) + sum(pixel * coeff)) >> 22, 0, 255), the horizontal pass into a uint8 intermediate.
 * colour_tab (UENC_AUG_COLOUR_TAB_INTS ints) may be NULL with colour_flags == 0: no colour stage.  hue in (-180, 180).
 * -1: a null / misaligned pointer, an empty size, a window outside the resized image, or a plan whose tile does not fit (see above). */
int uenc_augment_image(const unsigned char* src, long frame_stride, int F, int in_h, int in_w, int rs_h, int rs_w, int x0, int y0, int cw,
                       int ch, const int* col_tab, int kx, const int* row_tab, int ky, const int* colour_tab, int colour_flags, int hue,
                       int flip, int out_h, int out_w, int pad_value, unsigned char* dst, uenc_stream_t stream);
/* pan_out (out_h, out_w) int32 = r + 256 g + 65536 b of the panoptic PNG pan (in_h, in_w, 3) uint8 at [pan_row[y], pan_col[x]], 0 in the
 * padding; label_out (out_h, out_w) int32 = label[lab_row[y], lab_col[x]] (label_bytes 1: uint8, 4: int32), ignore_label in the padding.
 * The tables hold SOURCE indices of the window's ch rows / cw columns (nearest resize; the two maps follow different libraries' rounding).
 * label, lab_col, lab_row and label_out may all be NULL: no label map. */
int uenc_augment_labels(const unsigned char* pan, const void* label, int label_bytes, int in_h, int in_w, int rs_h, int rs_w, int x0, int y0,
                        int cw, int ch, const int* pan_col, const int* pan_row, const int* lab_col, const int* lab_row, int flip, int out_h,
                        int out_w, int ignore_label, int* pan_out, int* label_out, uenc_stream_t stream);

/* ---- launch timers (opt-in, process-global): per-launch HIP events on the launch stream ---------------- */
int uenc_prof_enable(int on); /* also resets */
int uenc_prof_collect(int kind /* 0 gemm_nt (128-tile, skinny), 1 gemm_tn*, 4 gemm_nt256, 5 gemm_nt128 */, double* ms_total, double* flops_total, long* launches);
/* algorithmic bytes (operands read once + results written once) of the recorded launches of `kind` (gemm_nt kinds). */
int uenc_prof_collect_bytes(int kind, double* bytes_total);
/* algorithmic bytes of the NEXT recorded launch whose entry point cannot derive them (the grouped wgrad launches read their
 * problem sizes from a device table the caller built). */
int uenc_prof_next_bytes(double bytes);
/* 1 while the launch timers are on (a captured graph would replay their event records: uenc/graphs.py refuses to capture then). */
int uenc_prof_active(void);

#ifdef __cplusplus
}
#endif
#endif /* UENC_H */
