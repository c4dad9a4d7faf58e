// Evaluation statistics accumulated on the device (uenc/evaluation.py: SemSegEvaluator and PanopticEvaluator with accumulate="device").
// The host evaluators copy a label map per image to the CPU and count there; these kernels count where the maps already are and leave
// a few KB per image to be read once, at the end of the dataset.
//
//   uenc_eval_confusion     conf[pred, gt] += 1 per pixel of every image's own (h_b, w_b); pred = argmax over the C score planes (done
//                           here, lowest class wins a tie, the first NaN wins like torch.argmax) or, with C == 0, a label map
//   uenc_eval_pq_intersect  inter[b, row(gt id), col(pred id)] += 1 per pixel: the segment intersection matrix of panopticapi's pq_compute
//   uenc_eval_pq_match      panopticapi's matching rules on that matrix, one workgroup per image, integers only
//
// The first two walk one padded batch (B, H, W) with grid (chunks, B) like targets.hip: a workgroup serves chunks of 4096 pixels of ONE
// image, grid-stride beyond `max_blocks` workgroups per image.  A thread takes four groups of four consecutive pixels per chunk, group q
// at chunk + 1024 q + 4 tid, so that every 16-byte load of a wave covers 1 KiB of consecutive addresses; when H * W is no multiple of 4
// or a map is not 16-byte aligned, a lane takes one pixel at a time and consecutive lanes consecutive pixels.
//
// Bound: HBM reads.  The confusion kernel reads (C + 1) * 4 bytes per pixel once (C planes of scores and the ground truth) and stores
// nothing per pixel; the intersect kernel reads 8 bytes per pixel.  The counting must stay off that path:
//   * every thread counts runs of equal cells first (both maps are piecewise constant) and issues one integer atomic per run;
//   * confusion: while (N + 1)^2 <= 4096 counters (N <= 63: 16 KB, eight workgroups per CU still fit) the histogram is private to the
//     workgroup in LDS and flushed with one 64-bit global atomic per non-zero cell; above that (N = 150 would take 91 KB of the 160 KB and
//     leave one workgroup per CU to hide the load latency) the runs go to global memory directly, which piecewise-constant maps keep few;
//   * intersect: a full 258 x 258 int32 matrix is 266 KB and cannot live in LDS, but a workgroup's 4096-pixel chunks meet only a
//     handful of (row, col) pairs.  A 1024-slot pair table in LDS (8 KB) sits in front of global memory: a run claims the slot its cell
//     hashes to, or finds its own cell there, and adds in LDS; a run whose slot is taken by another cell goes to global memory
//     at once.  The table is flushed once per workgroup, so a 1024 x 2048 image costs a few thousand global atomics instead of one per
//     run (>= 131072, most of them on the same few addresses of one L2 channel).
// All accumulation is integer atomics (LDS and global): sums do not depend on the order, two calls give the same bits.  No float
// atomics, nothing is read back.  Values that index memory (sizes, n_gt, n_pred, categories) are clamped or checked on the device.
#include "common.h"
#include "tg_table.h"

#define EV_DIM (TG_ROWS + 2)               // UENC_EVAL_PQ_DIM: VOID, 256 table rows, "unknown"
#define EV_LDS_CELLS 4096                  // confusion cells counted in LDS
#define EV_PAIRS 1024                      // slots of the intersect kernel's LDS pair table
#define EV_MAX_CLASSES 1024                // UENC_EVAL_MAX_CLASSES

static_assert(EV_DIM == UENC_EVAL_PQ_DIM && EV_MAX_CLASSES == UENC_EVAL_MAX_CLASSES && TG_ROWS == UENC_TARGETS_MAX_SEGMENTS, "include/uenc.h");

// The pixels of one thread: f(p, y, x, vec) per group of four (vec, p % 4 == 0, all four inside H * W) or per pixel.
template <bool VEC, class F>
__device__ __forceinline__ void ev_walk(int HW, int W, F f) {
    const int chunks = (HW + TG_CHUNK - 1) / TG_CHUNK;
    for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
        if (VEC) {
#pragma unroll
            for (int q = 0; q < TG_PIX / 4; ++q) {
                const int p0 = c * TG_CHUNK + q * (4 * TG_THREADS) + 4 * threadIdx.x;
                if (p0 < HW) f(p0);                                         // HW % 4 == 0: a group is all in or all out
            }
        } else {
            for (int i = 0; i < TG_PIX; ++i) {
                const int p = c * TG_CHUNK + i * TG_THREADS + threadIdx.x;
                if (p >= HW) break;
                f(p);
            }
        }
    }
}

__device__ __forceinline__ void ev_argmax_step(float& best, int& arg, float v, int c) {
    if (v > best || (v != v && best == best)) {                             // strict: the lowest index keeps a tie; the first NaN stays
        best = v;
        arg = c;
    }
}

// ---- confusion matrix ---------------------------------------------------------------------------------------------------------------------
template <bool VEC, bool LDSH>
__global__ __launch_bounds__(TG_THREADS) void eval_confusion_kernel(const float* __restrict__ scores, const int* __restrict__ labels,
                                                                    const int* __restrict__ gt, const int* __restrict__ sizes,
                                                                    unsigned long long* __restrict__ conf, int C, int N, int ignore_label,
                                                                    int H, int W) {
    __shared__ int hist[LDSH ? EV_LDS_CELLS : 1];
    const int b = blockIdx.y;
    const int h = tg_clamp(sizes[2 * b], 0, H), w = tg_clamp(sizes[2 * b + 1], 0, W);
    const int N1 = N + 1, cells = N1 * N1;
    if (LDSH) {
        for (int i = threadIdx.x; i < cells; i += TG_THREADS) hist[i] = 0;
        __syncthreads();
    }
    const int HW = H * W;
    const float* __restrict__ sc = scores ? scores + (size_t)b * C * HW : nullptr;
    const int* __restrict__ lab = labels ? labels + (size_t)b * HW : nullptr;
    const int* __restrict__ g = gt + (size_t)b * HW;

    int run_cell = -1, run = 0;
    auto flush = [&]() {
        if (run_cell < 0) return;
        if (LDSH) atomicAdd(&hist[run_cell], run);
        else atomicAdd(&conf[run_cell], (unsigned long long)run);
    };
    auto count = [&](int pred, int truth) {
        const int pr = (unsigned)pred < (unsigned)N ? pred : N;
        const int tc = (truth != ignore_label && (unsigned)truth < (unsigned)N) ? truth : N;
        const int cell = pr * N1 + tc;
        if (cell != run_cell) {
            flush();
            run_cell = cell;
            run = 0;
        }
        ++run;
    };
    ev_walk<VEC>(HW, W, [&](int p) {
        int y = p / W, x = p - y * W;
        if (VEC) {
            const int4 tv = *reinterpret_cast<const int4*>(g + p);
            const int truth[4] = {tv.x, tv.y, tv.z, tv.w};
            int arg[4] = {0, 0, 0, 0};
            if (sc) {
                float4 best = *reinterpret_cast<const float4*>(sc + p);
#pragma unroll 4
                for (int c = 1; c < C; ++c) {
                    const float4 v = *reinterpret_cast<const float4*>(sc + (size_t)c * HW + p);
                    ev_argmax_step(best.x, arg[0], v.x, c);
                    ev_argmax_step(best.y, arg[1], v.y, c);
                    ev_argmax_step(best.z, arg[2], v.z, c);
                    ev_argmax_step(best.w, arg[3], v.w, c);
                }
            } else {
                const int4 lv = *reinterpret_cast<const int4*>(lab + p);
                arg[0] = lv.x; arg[1] = lv.y; arg[2] = lv.z; arg[3] = lv.w;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (y < h && x < w) count(arg[i], truth[i]);
                if (++x == W) { x = 0; ++y; }
            }
        } else {
            if (y >= h || x >= w) return;
            int arg = 0;
            if (sc) {
                float best = sc[p];
                for (int c = 1; c < C; ++c) ev_argmax_step(best, arg, sc[(size_t)c * HW + p], c);
            } else {
                arg = lab[p];
            }
            count(arg, g[p]);
        }
    });
    flush();
    if (LDSH) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += TG_THREADS) {
            const int v = hist[i];
            if (v) atomicAdd(&conf[i], (unsigned long long)v);
        }
    }
}

// ---- panoptic quality: intersection matrix ------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(TG_THREADS) void eval_pq_intersect_kernel(const int* __restrict__ pred, const int* __restrict__ gt,
                                                                       const int* __restrict__ sizes, const int* __restrict__ gt_ids,
                                                                       const int* __restrict__ n_gt, const int* __restrict__ pred_ids,
                                                                       const int* __restrict__ n_pred, int* __restrict__ inter, int H, int W) {
    __shared__ TgTable tbg, tbp;
    __shared__ int pkey[EV_PAIRS], pcnt[EV_PAIRS];
    const int b = blockIdx.y;
    const int ng = tg_clamp(n_gt[b], 0, TG_ROWS), np = tg_clamp(n_pred[b], 0, TG_ROWS);
    const int h = tg_clamp(sizes[2 * b], 0, H), w = tg_clamp(sizes[2 * b + 1], 0, W);
    for (int i = threadIdx.x; i < EV_PAIRS; i += TG_THREADS) {
        pkey[i] = -1;
        pcnt[i] = 0;
    }
    tg_build(tbg, gt_ids + (size_t)b * TG_ROWS, ng);                        // its barriers cover the pair table as well
    tg_build(tbp, pred_ids + (size_t)b * TG_ROWS, np);

    const int HW = H * W;
    const int* __restrict__ pm = pred + (size_t)b * HW;
    const int* __restrict__ gm = gt + (size_t)b * HW;
    int* __restrict__ out = inter + (size_t)b * EV_DIM * EV_DIM;
    TgLast lastg, lastp;
    int run_cell = -1, run = 0;
    auto flush = [&]() {
        if (run_cell < 0) return;
        const unsigned s = ((unsigned)run_cell * 2654435761u) >> 22;       // 10 bits
        const int old = atomicCAS(&pkey[s], -1, run_cell);
        if (old == -1 || old == run_cell) atomicAdd(&pcnt[s], run);
        else atomicAdd(&out[run_cell], run);
    };
    auto count = [&](int pid, int gid) {
        int r = 0, c = 0;                                                   // id 0 is VOID; an id without a table row is "unknown"
        if (gid != 0) {
            const int k = lastg(tbg, gid);
            r = k >= 0 ? k + 1 : ng + 1;
        }
        if (pid != 0) {
            const int k = lastp(tbp, pid);
            c = k >= 0 ? k + 1 : np + 1;
        }
        const int cell = r * EV_DIM + c;
        if (cell != run_cell) {
            flush();
            run_cell = cell;
            run = 0;
        }
        ++run;
    };
    ev_walk<VEC>(HW, W, [&](int p) {
        int y = p / W, x = p - y * W;
        if (VEC) {
            const int4 pv = *reinterpret_cast<const int4*>(pm + p);
            const int4 gv = *reinterpret_cast<const int4*>(gm + p);
            const int pid[4] = {pv.x, pv.y, pv.z, pv.w}, gid[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (y < h && x < w) count(pid[i], gid[i]);
                if (++x == W) { x = 0; ++y; }
            }
        } else if (y < h && x < w) {
            count(pm[p], gm[p]);
        }
    });
    flush();
    __syncthreads();
    for (int i = threadIdx.x; i < EV_PAIRS; i += TG_THREADS) {
        const int v = pcnt[i];
        if (v) atomicAdd(&out[pkey[i]], v);
    }
}

// ---- panoptic quality: matching -----------------------------------------------------------------------------------------------------------
// One workgroup per image; thread t owns ground-truth row t + 1 and predicted column t + 1 of the image's matrix.  The matrix is read
// twice with consecutive lanes on consecutive cells (it is sparse: a cell > 0 per pair of overlapping segments), first for the areas
// (row and column sums), then for the pairs: IoU > 0.5 is 2 * inter > union in 64-bit integers, so at most one column matches a row
// and one row a column, and plain stores record the match.
__global__ __launch_bounds__(TG_THREADS) void eval_pq_match_kernel(const int* __restrict__ inter, const int* __restrict__ n_gt,
                                                                   const int* __restrict__ n_pred, const int* __restrict__ gt_cat,
                                                                   const int* __restrict__ gt_crowd, const int* __restrict__ pred_cat,
                                                                   int* __restrict__ rec, int* __restrict__ fp, int* __restrict__ fn,
                                                                   int* __restrict__ unknown, int K) {
    __shared__ int area_g[EV_DIM], area_p[EV_DIM], crowd_p[EV_DIM], hit_p[EV_DIM];
    __shared__ int m_col[EV_DIM], m_inter[EV_DIM], m_union[EV_DIM];
    __shared__ int s_gcat[TG_ROWS], s_gcrowd[TG_ROWS], s_pcat[TG_ROWS];
    __shared__ int s_fp[EV_MAX_CLASSES], s_fn[EV_MAX_CLASSES];
    const int b = blockIdx.x, t = threadIdx.x;
    const int ng = tg_clamp(n_gt[b], 0, TG_ROWS), np = tg_clamp(n_pred[b], 0, TG_ROWS);
    const int* __restrict__ M = inter + (size_t)b * EV_DIM * EV_DIM;
    for (int i = t; i < EV_DIM; i += TG_THREADS) {
        area_g[i] = area_p[i] = crowd_p[i] = hit_p[i] = 0;
        m_col[i] = -1;
        m_inter[i] = m_union[i] = 0;
    }
    s_gcat[t] = t < ng ? gt_cat[(size_t)b * TG_ROWS + t] : -1;
    s_gcrowd[t] = t < ng ? gt_crowd[(size_t)b * TG_ROWS + t] != 0 : 0;
    s_pcat[t] = t < np ? pred_cat[(size_t)b * TG_ROWS + t] : -1;
    for (int i = t; i < K; i += TG_THREADS) s_fp[i] = s_fn[i] = 0;
    __syncthreads();

    // areas: a predicted segment's includes its pixels over VOID (row 0) and over unknown ground truth (row ng + 1)
    for (int i = t; i < (ng + 2) * EV_DIM; i += TG_THREADS) {
        const int r = i / EV_DIM, c = i - r * EV_DIM;
        if (c > np + 1) continue;
        const int v = M[i];
        if (v > 0) {
            atomicAdd(&area_g[r], v);
            atomicAdd(&area_p[c], v);
        }
    }
    __syncthreads();
    // candidate pairs: real segments on both sides, same category; a crowd never matches, its overlap counts towards the column's FP rule
    for (int i = EV_DIM + t; i < (ng + 1) * EV_DIM; i += TG_THREADS) {
        const int r = i / EV_DIM, c = i - r * EV_DIM;
        if (c < 1 || c > np) continue;
        const int v = M[i];
        if (v <= 0 || s_gcat[r - 1] != s_pcat[c - 1]) continue;
        if (s_gcrowd[r - 1]) {
            atomicAdd(&crowd_p[c], v);
            continue;
        }
        const long long uni = (long long)area_p[c] + area_g[r] - v - M[c];
        if (2ll * v > uni) {
            m_col[r] = c - 1;
            m_inter[r] = v;
            m_union[r] = (int)uni;
            hit_p[c] = 1;
        }
    }
    __syncthreads();
    {
        int* __restrict__ o = rec + ((size_t)b * TG_ROWS + t) * 4;
        const int r = t + 1, cat = s_gcat[t];
        o[0] = t < ng ? m_col[r] : -1;
        o[1] = t < ng ? m_inter[r] : 0;
        o[2] = t < ng ? m_union[r] : 0;
        o[3] = cat;
        if (t < ng && m_col[r] < 0 && !s_gcrowd[t] && area_g[r] > 0 && (unsigned)cat < (unsigned)K) atomicAdd(&s_fn[cat], 1);
    }
    if (t < np && !hit_p[t + 1]) {
        const int c = t + 1, cat = s_pcat[t];
        const long long v = (long long)M[c] + crowd_p[c];                   // over VOID and over crowds of its own category
        if (!(2 * v > (long long)area_p[c]) && (unsigned)cat < (unsigned)K) atomicAdd(&s_fp[cat], 1);
    }
    if (t == 0) unknown[b] = area_p[np + 1];
    __syncthreads();
    for (int i = t; i < K; i += TG_THREADS) {
        fp[(size_t)b * K + i] = s_fp[i];
        fn[(size_t)b * K + i] = s_fn[i];
    }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------------
static inline bool ev_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static inline bool ev_batch_ok(int B, int H, int W, int max_blocks) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= 0x7fffffff - TG_CHUNK && max_blocks >= 0;
}

static inline int ev_blocks(int H, int W, int max_blocks) {
    const int blocks = tg_blocks(H, W);
    return (max_blocks > 0 && max_blocks < blocks) ? max_blocks : blocks;
}

extern "C" int uenc_eval_confusion(const void* pred, const int* gt, const int* sizes, long long* conf, int B, int C, int H, int W,
                                   int num_classes, int ignore_label, int max_blocks, hipStream_t stream) {
    UENC_CHECK_ARG(pred && gt && sizes && conf);
    UENC_CHECK_ARG(ev_aligned(pred, 4) && ev_aligned(gt, 4) && ev_aligned(sizes, 4) && ev_aligned(conf, 8));
    UENC_CHECK_ARG(ev_batch_ok(B, H, W, max_blocks) && C >= 0 && C <= EV_MAX_CLASSES && num_classes >= 1 && num_classes <= EV_MAX_CLASSES);
    UENC_CHECK_ARG((int64_t)B * (C > 0 ? C : 1) * H * W <= ((int64_t)1 << 40));
    const dim3 grid(ev_blocks(H, W, max_blocks), B), block(TG_THREADS);
    const float* scores = C > 0 ? (const float*)pred : nullptr;
    const int* labels = C > 0 ? nullptr : (const int*)pred;
    unsigned long long* out = (unsigned long long*)conf;
    const bool vec = ((int64_t)H * W) % 4 == 0 && ev_aligned(pred, 16) && ev_aligned(gt, 16);
    const bool lds = (num_classes + 1) * (num_classes + 1) <= EV_LDS_CELLS;
#define EV_CONF(V, L) \
    hipLaunchKernelGGL((eval_confusion_kernel<V, L>), grid, block, 0, stream, scores, labels, gt, sizes, out, C, num_classes, ignore_label, H, W)
    if (vec && lds) EV_CONF(true, true);
    else if (vec) EV_CONF(true, false);
    else if (lds) EV_CONF(false, true);
    else EV_CONF(false, false);
#undef EV_CONF
    UENC_LAUNCH_RET();
}

extern "C" int uenc_eval_pq_intersect(const int* pred, const int* gt, const int* sizes, const int* gt_ids, const int* n_gt, const int* pred_ids,
                                      const int* n_pred, int* inter, int B, int H, int W, int max_blocks, hipStream_t stream) {
    UENC_CHECK_ARG(pred && gt && sizes && gt_ids && n_gt && pred_ids && n_pred && inter);
    UENC_CHECK_ARG(ev_aligned(pred, 4) && ev_aligned(gt, 4) && ev_aligned(sizes, 4) && ev_aligned(gt_ids, 4) && ev_aligned(n_gt, 4) &&
                   ev_aligned(pred_ids, 4) && ev_aligned(n_pred, 4) && ev_aligned(inter, 4));
    UENC_CHECK_ARG(ev_batch_ok(B, H, W, max_blocks));
    const dim3 grid(ev_blocks(H, W, max_blocks), B), block(TG_THREADS);
    if (((int64_t)H * W) % 4 == 0 && ev_aligned(pred, 16) && ev_aligned(gt, 16))
        hipLaunchKernelGGL(eval_pq_intersect_kernel<true>, grid, block, 0, stream, pred, gt, sizes, gt_ids, n_gt, pred_ids, n_pred, inter, H, W);
    else
        hipLaunchKernelGGL(eval_pq_intersect_kernel<false>, grid, block, 0, stream, pred, gt, sizes, gt_ids, n_gt, pred_ids, n_pred, inter, H, W);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_eval_pq_match(const int* inter, const int* n_gt, const int* n_pred, const int* gt_cat, const int* gt_crowd,
                                  const int* pred_cat, int* rec, int* fp, int* fn, int* unknown, int B, int K, hipStream_t stream) {
    UENC_CHECK_ARG(inter && n_gt && n_pred && gt_cat && gt_crowd && pred_cat && rec && fp && fn && unknown);
    UENC_CHECK_ARG(ev_aligned(inter, 4) && ev_aligned(n_gt, 4) && ev_aligned(n_pred, 4) && ev_aligned(gt_cat, 4) && ev_aligned(gt_crowd, 4) &&
                   ev_aligned(pred_cat, 4) && ev_aligned(rec, 4) && ev_aligned(fp, 4) && ev_aligned(fn, 4) && ev_aligned(unknown, 4));
    UENC_CHECK_ARG(B >= 1 && B <= 65535 && K >= 1 && K <= EV_MAX_CLASSES);
    hipLaunchKernelGGL(eval_pq_match_kernel, dim3(B), dim3(TG_THREADS), 0, stream, inter, n_gt, n_pred, gt_cat, gt_crowd, pred_cat, rec, fp, fn,
                       unknown, K);
    UENC_LAUNCH_RET();
}
