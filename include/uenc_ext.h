/* libuenc_hip.so — extension entry points: what joins the library after include/uenc.h, the core ABI, was frozen.
 *
 * Same conventions as uenc.h: plain device pointers and sizes, 0 = launched, < 0 = invalid argument (nothing was launched, no HIP
 * call was made), > 0 = hipError_t; the caller owns every buffer, the library allocates nothing and never synchronises; everything
 * is enqueued on the given stream.  Definitions live in uni-encoder-code_amd/csrc/ext/ and are compiled against this header.
 * uenc/capi.py binds these declarations on the same library object as EXT_FUNCTIONS / EXT_CONSTANTS.
 */
#ifndef UENC_EXT_H
#define UENC_EXT_H
#include "uenc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dtype tag of a double-precision operand, beside UENC_F32 = 0 and UENC_BF16 = 1 of uenc.h */
#define UENC_EXT_F64 2

/* ---- depth evaluation on the device (csrc/ext/depth_eval.hip; uenc/evaluation.py: the depth evaluators with accumulate="device") ----
 * One row of the result buffer, in doubles: abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, then n = the number of valid pixels, the
 * median of the valid ground truth, the median of the valid predictions, and the three threshold counts n * a1, n * a2, n * a3. */
#define UENC_DEPTH_EVAL_ROW 13
/* kernels one uenc_depth_eval_score call enqueues behind its one hipMemsetAsync, by ground-truth dtype */
#define UENC_DEPTH_EVAL_LAUNCHES_F32 6
#define UENC_DEPTH_EVAL_LAUNCHES_F64 10

/* pred (H, W) = 1 / resize(disp (h, w)) in fp32: bilinear taps at half-pixel centres (cv2 INTER_LINEAR = F.interpolate(mode="bilinear",
 * align_corners=False)), coordinate, weights and lerps in fp64 from the fp32 taps, one rounding to fp32, then an IEEE division.
 * `resized`, when not NULL, receives the (H, W) resized disparity before the division.  One kernel. */
int uenc_depth_eval_pred(const float* disp, float* pred, float* resized, int h, int w, int H, int W, uenc_stream_t stream);

/* Bytes of workspace uenc_depth_eval_score needs for an (H, W) map and any window inside it; < 0 for a non-positive or too large size. */
long uenc_depth_eval_ws_bytes(int H, int W);

/* Scores one image: valid = inside the window [r0, r1) x [c0, c1) and min_depth < gt < max_depth (compared in gt's precision);
 * exact medians (numpy's definition) of gt[valid] (fp64) and pred[valid] (fp32); p = clamp(pred * med_gt / med_pred, min, max);
 * the seven metrics of `compute_errors` in fp64.  Writes rows[row * UENC_DEPTH_EVAL_ROW ...]; no valid pixel gives NaN metrics
 * and n = 0.  gt is (H, W) fp32 (gt_dtype = UENC_F32) or fp64 (UENC_EXT_F64), pred (H, W) fp32; `ws` holds at least
 * uenc_depth_eval_ws_bytes(H, W) bytes, 8-byte aligned, contents irrelevant before and undefined after; 0 <= row < capacity.
 * No float atomics: two calls on the same input write the same bits. */
int uenc_depth_eval_score(const void* gt, int gt_dtype, const float* pred, int H, int W, int r0, int r1, int c0, int c1,
                          double min_depth, double max_depth, void* ws, long ws_bytes, double* rows, int row, int capacity,
                          uenc_stream_t stream);

/* ---- neighbourhood attention: what the planner of uenc_na2d_fwd / uenc_na2d_bwd decides (csrc/ext/na2d_plan.hip; host code only) ----
 * The number of consecutive tiles of a residue class one workgroup of the matrix-core kernels walks for this problem, 0 where the
 * VALU kernels run instead (K >= 9, or a per-image qkv extent of 2^31 elements or more), < 0 for arguments uenc_na2d_fwd refuses.
 * Nothing is launched.  tests/na2d_cases.py restates the planner and is held against this. */
int uenc_na2d_tiles_per_group(int B, int H, int W, int nH, int K, int dilation);

#ifdef __cplusplus
}
#endif
#endif /* UENC_EXT_H */
