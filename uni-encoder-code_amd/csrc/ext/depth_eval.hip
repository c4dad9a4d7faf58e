// Depth evaluation on the device (uenc/evaluation.py: KITTIDepthEvaluator and CityscapesDepthEvaluator with accumulate="device").
// The host evaluators copy every disparity map to the CPU, resize it there, boolean-index two full-resolution maps, take two
// np.median and keep both maps until evaluate(); these kernels leave UENC_DEPTH_EVAL_ROW doubles per image on the device.
//
//   uenc_depth_eval_pred    pred = 1 / bilinear_resize(disp): one thread per output pixel, fp64 taps, one rounding, IEEE division
//   uenc_depth_eval_score   valid set -> exact medians of gt[valid] and pred[valid] -> the seven metrics of compute_errors
//
// The score is a chain of small kernels over the scoring window only (at most 512 x 1664 pixels of Cityscapes, 12 bytes each: the
// window stays in L2 between the passes, the chain is launch- and latency-bound, not bandwidth-bound):
//   * NP histogram passes of an MSB-first radix select with 8-bit digits, NP = 4 for fp32 ground truth, 8 for fp64 (32- and 64-bit
//     keys; the fp32 predictions finish after 4).  A float's key is its bit pattern with the sign bit flipped (positive) or all bits
//     flipped (negative): unsigned key order = float order for every non-NaN value.  Four selections run through the same passes:
//     ranks (n - 1) / 2 and n / 2 of either array, which are one rank when n is odd; while the two prefixes of an array agree (always
//     in pass 0, nearly always later) the array counts into one histogram and both ranks read it.
//   * A pass counts in a workgroup's LDS (4 x 256 ints, integer LDS atomics) and flushes non-zero bins with integer global atomics.
//     The valid mask is not stored: every pass re-derives it from gt, and pass 0's histogram total IS n.
//   * There is no select kernel: every workgroup of pass p + 1 (and of the metric kernel) reads pass p's 4 x 256 global counts and
//     advances the selection state itself, one wave per selection (four bins per lane, a wave scan, a ballot); workgroup 0 stores the
//     state for the next kernel.  n, ranks and prefixes never leave the device.
//   * The metric kernel accumulates per thread in pixel order, reduces in a fixed butterfly per wave and over the four waves in
//     order, and stores one partial per workgroup; the last kernel adds the partials in index order and writes the row.  The grid
//     depends on the window area alone, so equal inputs give equal bits.  No float atomics.
// Launches per image: 1 (pred) + one memset of the histograms + NP + 2 = 8 for fp32, 12 for fp64 ground truth.
#include "../common.h"
#include "../../../include/uenc_ext.h"

#define DE_THREADS 256
#define DE_ELEMS 8
#define DE_CHUNK (DE_THREADS * DE_ELEMS)          // window pixels per workgroup and grid step
#define DE_MAX_BLOCKS 1024                       // grid-stride beyond that; the partials of the metric kernel are sized by it
#define DE_MAX_PASSES 8
#define DE_HIST_INTS (4 * 256)                    // gt lo, gt hi, pred lo, pred hi
#define DE_MAX_PIXELS (1 << 30)

struct DeState {                                  // after p passes: p leading digits of each selection, the rank left inside them
    unsigned long long gprefix[2];
    unsigned grank[2];
    unsigned pprefix[2];
    unsigned prank[2];
    unsigned n, pad;
};

// workspace: histograms of every pass | states 0 .. NP | n and the medians | one partial of 8 doubles per workgroup
#define DE_STATE_OFF (DE_MAX_PASSES * DE_HIST_INTS * 4)
#define DE_FINAL_OFF (DE_STATE_OFF + 1024)
#define DE_PART_OFF (DE_FINAL_OFF + 64)
static_assert((DE_MAX_PASSES + 1) * sizeof(DeState) <= 1024 && sizeof(DeState) % 8 == 0, "workspace layout");
static_assert(UENC_DEPTH_EVAL_LAUNCHES_F32 == 4 + 2 && UENC_DEPTH_EVAL_LAUNCHES_F64 == 8 + 2 && UENC_DEPTH_EVAL_ROW == 13, "include/uenc_ext.h");

template <class T> struct DeKey;
template <> struct DeKey<float> {
    typedef unsigned K;
    static constexpr int BITS = 32;
    static __device__ __forceinline__ K key(float v) {
        const unsigned u = __float_as_uint(v);
        return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
    }
    static __device__ __forceinline__ float val(K k) { return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }
};
template <> struct DeKey<double> {
    typedef unsigned long long K;
    static constexpr int BITS = 64;
    static __device__ __forceinline__ K key(double v) {
        const unsigned long long u = (unsigned long long)__double_as_longlong(v);
        return u ^ ((u >> 63) ? 0xffffffffffffffffull : 0x8000000000000000ull);
    }
    static __device__ __forceinline__ double val(K k) { return __longlong_as_double((long long)((k >> 63) ? k ^ 0x8000000000000000ull : ~k)); }
};

static inline int de_blocks(int64_t area) {
    const int64_t b = (area + DE_CHUNK - 1) / DE_CHUNK;
    return (int)(b < DE_MAX_BLOCKS ? b : DE_MAX_BLOCKS);
}

// f(i) for the window pixels of this thread, i = row-major index inside the window; consecutive lanes take consecutive pixels
template <class F>
__device__ __forceinline__ void de_walk(int area, F f) {
    const int chunks = (area + DE_CHUNK - 1) / DE_CHUNK;
    for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
#pragma unroll
        for (int k = 0; k < DE_ELEMS; ++k) {
            const int i = c * DE_CHUNK + k * DE_THREADS + (int)threadIdx.x;
            if (i < area) f(i);
        }
    }
}

struct DeWindow {
    int W, r0, c0, ww, area;
    __device__ __forceinline__ size_t at(int i) const {
        const int r = i / ww;
        return (size_t)(r0 + r) * W + (c0 + i - r * ww);
    }
};

// st <- the state after p passes, from the state after p - 1 (stored by workgroup 0 of the previous kernel) and pass p - 1's global
// histograms.  Wave w advances selection w (0 gt lo, 1 gt hi, 2 pred lo, 3 pred hi).  `h` is scratch; ends behind a barrier.
template <class GT>
__device__ void de_advance(DeState& st, unsigned* h, const unsigned* __restrict__ hist_all, DeState* __restrict__ states, int p) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (p == 0) {
        if (tid == 0) {
            st.gprefix[0] = st.gprefix[1] = 0;
            st.grank[0] = st.grank[1] = st.pprefix[0] = st.pprefix[1] = st.prank[0] = st.prank[1] = st.n = st.pad = 0;
            if (blockIdx.x == 0) states[0] = st;
        }
        __syncthreads();
        return;
    }
    const int q = p - 1;                                                    // the pass whose counts are read
    for (int i = tid; i < DE_HIST_INTS; i += DE_THREADS) h[i] = hist_all[(size_t)q * DE_HIST_INTS + i];
    if (tid == 0) st = states[q];
    __syncthreads();
    const bool is_pred = wave >= 2;
    const int side = wave & 1;
    const bool same = is_pred ? st.pprefix[0] == st.pprefix[1] : st.gprefix[0] == st.gprefix[1];
    const bool active = q < (is_pred ? 4 : DeKey<GT>::BITS / 8);
    const unsigned* hh = h + ((wave & 2) + (same ? 0 : side)) * 256;
    const unsigned c0 = hh[4 * lane], c1 = hh[4 * lane + 1], c2 = hh[4 * lane + 2], c3 = hh[4 * lane + 3];
    const unsigned s = c0 + c1 + c2 + c3;
    unsigned incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    const unsigned total = __shfl(incl, 63);
    unsigned n = st.n;
    unsigned rank = is_pred ? st.prank[side] : st.grank[side];
    if (q == 0) {                                                           // pass 0 counted every valid pixel: its total is n
        n = total;
        rank = side ? n / 2 : (n ? (n - 1) / 2 : 0);
    }
    const unsigned long long prefix = is_pred ? (unsigned long long)st.pprefix[side] : st.gprefix[side];
    const unsigned excl = incl - s;
    const unsigned long long pick = __ballot(rank >= excl && rank < incl);
    unsigned digit = 0, left = 0;
    if (pick) {                                                             // none: n == 0
        const int src = __ffsll((long long)pick) - 1;
        unsigned r = rank - excl, d = 0;
        if (r >= c0) { r -= c0; d = 1;
            if (r >= c1) { r -= c1; d = 2;
                if (r >= c2) { r -= c2; d = 3; } } }
        digit = __shfl(4 * lane + d, src);
        left = __shfl(r, src);
    }
    __syncthreads();                                                        // every wave has read st
    if (active && lane == 0) {
        if (is_pred) {
            st.pprefix[side] = (unsigned)(prefix << 8) | digit;
            st.prank[side] = left;
        } else {
            st.gprefix[side] = (prefix << 8) | digit;
            st.grank[side] = left;
        }
        if (wave == 0) st.n = n;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) states[p] = st;
}

// ---- one histogram pass --------------------------------------------------------------------------------------------------------------------
template <class GT>
__global__ __launch_bounds__(DE_THREADS) void de_hist_kernel(const GT* __restrict__ gt, const float* __restrict__ pred, DeWindow win, GT lo, GT hi,
                                                             unsigned* __restrict__ hist_all, DeState* __restrict__ states, int p) {
    typedef typename DeKey<GT>::K GK;
    constexpr int GB = DeKey<GT>::BITS;
    __shared__ unsigned h[DE_HIST_INTS];
    __shared__ DeState st;
    de_advance<GT>(st, h, hist_all, states, p);
    const unsigned long long gpre0 = st.gprefix[0], gpre1 = st.gprefix[1];
    const unsigned ppre0 = st.pprefix[0], ppre1 = st.pprefix[1];
    __syncthreads();
    for (int i = threadIdx.x; i < DE_HIST_INTS; i += DE_THREADS) h[i] = 0;
    __syncthreads();
    const bool g_on = p < GB / 8, p_on = p < 4;
    const int gshift = g_on ? GB - 8 * (p + 1) : 0, pshift = p_on ? 32 - 8 * (p + 1) : 0;
    de_walk(win.area, [&](int i) {
        const size_t o = win.at(i);
        const GT g = gt[o];
        if (!(g > lo && g < hi)) return;
        if (g_on) {
            const GK k = DeKey<GT>::key(g);
            const unsigned long long pre = p ? (unsigned long long)(k >> ((gshift + 8) & (GB - 1))) : 0ull;
            const unsigned d = (unsigned)(k >> gshift) & 255u;
            if (pre == gpre0) atomicAdd(&h[d], 1u);
            if (gpre0 != gpre1 && pre == gpre1) atomicAdd(&h[256 + d], 1u);
        }
        if (p_on) {
            const unsigned k = DeKey<float>::key(pred[o]);
            const unsigned pre = p ? k >> ((pshift + 8) & 31) : 0u;
            const unsigned d = (k >> pshift) & 255u;
            if (pre == ppre0) atomicAdd(&h[512 + d], 1u);
            if (ppre0 != ppre1 && pre == ppre1) atomicAdd(&h[768 + d], 1u);
        }
    });
    __syncthreads();
    unsigned* __restrict__ out = hist_all + (size_t)p * DE_HIST_INTS;
    for (int i = threadIdx.x; i < DE_HIST_INTS; i += DE_THREADS) {
        const unsigned v = h[i];
        if (v) atomicAdd(&out[i], v);
    }
}

// ---- metrics: per-workgroup partial sums --------------------------------------------------------------------------------------------------
__device__ __forceinline__ double de_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <class GT>
__global__ __launch_bounds__(DE_THREADS) void de_metric_kernel(const GT* __restrict__ gt, const float* __restrict__ pred, DeWindow win, GT lo, GT hi,
                                                               double dmin, double dmax, const unsigned* __restrict__ hist_all,
                                                               DeState* __restrict__ states, int np, double* __restrict__ fin,
                                                               double* __restrict__ partials) {
    __shared__ unsigned h[DE_HIST_INTS];
    __shared__ DeState st;
    __shared__ double red[DE_THREADS / 64][8];
    de_advance<GT>(st, h, hist_all, states, np);                            // the selections are complete: the prefixes are whole keys
    const double med_gt = ((double)DeKey<GT>::val((typename DeKey<GT>::K)st.gprefix[0]) + (double)DeKey<GT>::val((typename DeKey<GT>::K)st.gprefix[1])) * 0.5;
    const float med_pred = (DeKey<float>::val(st.pprefix[0]) + DeKey<float>::val(st.pprefix[1])) * 0.5f;
    const double ratio = med_gt / (double)med_pred;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};                               // abs_rel, sq_rel, sq, sq_log, then the three counts
    de_walk(win.area, [&](int i) {
        const size_t o = win.at(i);
        const GT gv = gt[o];
        if (!(gv > lo && gv < hi)) return;
        const double g = (double)gv;
        double q = (double)pred[o] * ratio;
        q = q < dmin ? dmin : (q > dmax ? dmax : q);                        // np.clip: a NaN stays a NaN
        const double diff = g - q, a = g / q, b = q / g;
        const double r = (a != a || b != b) ? a + b : (a > b ? a : b);      // np.maximum propagates a NaN
        const double dl = log(g) - log(q);
        acc[0] += fabs(diff) / g;
        acc[1] += diff * diff / g;
        acc[2] += diff * diff;
        acc[3] += dl * dl;
        acc[4] += r < 1.25 ? 1.0 : 0.0;
        acc[5] += r < 1.5625 ? 1.0 : 0.0;
        acc[6] += r < 1.953125 ? 1.0 : 0.0;
    });
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double v = de_wave_sum(acc[j]);
        if (lane == 0) red[wave][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        double v = red[0][threadIdx.x];
        for (int w = 1; w < DE_THREADS / 64; ++w) v += red[w][threadIdx.x];
        partials[(size_t)blockIdx.x * 8 + threadIdx.x] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        fin[0] = (double)st.n;
        fin[1] = med_gt;
        fin[2] = (double)med_pred;
    }
}

// ---- the row: partials added in index order ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void de_row_kernel(const double* __restrict__ fin, const double* __restrict__ partials, int blocks,
                                                    double* __restrict__ row) {
    __shared__ double sum[8];
    if (threadIdx.x < 8) {
        double v = 0.0;
        for (int b = 0; b < blocks; ++b) v += partials[(size_t)b * 8 + threadIdx.x];
        sum[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double n = fin[0], nan = __longlong_as_double(0x7ff8000000000000ll);
    if (n > 0.0) {
        row[0] = sum[0] / n;
        row[1] = sum[1] / n;
        row[2] = sqrt(sum[2] / n);
        row[3] = sqrt(sum[3] / n);
        row[4] = sum[4] / n;
        row[5] = sum[5] / n;
        row[6] = sum[6] / n;
        row[7] = n;
        row[8] = fin[1];
        row[9] = fin[2];
        row[10] = sum[4];
        row[11] = sum[5];
        row[12] = sum[6];
    } else {
        for (int j = 0; j < 7; ++j) row[j] = nan;
        row[7] = 0.0;
        row[8] = row[9] = nan;
        row[10] = row[11] = row[12] = 0.0;
    }
}

// ---- prediction: resize and invert --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void de_tap(int d, double scale, int in, int& i0, int& i1, double& w1) {
    double s = ((double)d + 0.5) * scale - 0.5;
    if (s < 0.0) s = 0.0;
    i0 = (int)s;                                                            // s >= 0: truncation is floor
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + 1 < in ? i0 + 1 : in - 1;
    w1 = s - (double)i0;
}

__global__ __launch_bounds__(DE_THREADS) void de_pred_kernel(const float* __restrict__ disp, float* __restrict__ pred, float* __restrict__ resized,
                                                             int h, int w, int H, int W, double sy, double sx) {
    const int i = blockIdx.x * DE_THREADS + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    int y0, y1, x0, x1;
    double wy, wx;
    de_tap(y, sy, h, y0, y1, wy);
    de_tap(x, sx, w, x0, x1, wx);
    const double a = disp[(size_t)y0 * w + x0], b = disp[(size_t)y0 * w + x1], c = disp[(size_t)y1 * w + x0], d = disp[(size_t)y1 * w + x1];
    const double top = a * (1.0 - wx) + b * wx, bot = c * (1.0 - wx) + d * wx;
    const float v = (float)(top * (1.0 - wy) + bot * wy);
    if (resized) resized[i] = v;
    pred[i] = 1.0f / v;
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------------
static inline bool de_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static inline bool de_size_ok(int H, int W) { return H >= 1 && W >= 1 && (int64_t)H * W <= DE_MAX_PIXELS; }

extern "C" int uenc_depth_eval_pred(const float* disp, float* pred, float* resized, int h, int w, int H, int W, hipStream_t stream) {
    UENC_CHECK_ARG(disp && pred && de_aligned(disp, 4) && de_aligned(pred, 4) && de_aligned(resized, 4));
    UENC_CHECK_ARG(de_size_ok(h, w) && de_size_ok(H, W));
    const int blocks = (int)(((int64_t)H * W + DE_THREADS - 1) / DE_THREADS);
    hipLaunchKernelGGL(de_pred_kernel, dim3(blocks), dim3(DE_THREADS), 0, stream, disp, pred, resized, h, w, H, W, (double)h / (double)H,
                       (double)w / (double)W);
    UENC_LAUNCH_RET();
}

extern "C" long uenc_depth_eval_ws_bytes(int H, int W) {
    UENC_CHECK_ARG(de_size_ok(H, W));
    return (long)DE_PART_OFF + (long)de_blocks((int64_t)H * W) * 8 * (long)sizeof(double);
}

template <class GT>
static int de_score(const void* gt_, const float* pred, DeWindow win, double dmin, double dmax, char* ws, double* row, hipStream_t stream) {
    const GT* gt = (const GT*)gt_;
    constexpr int np = DeKey<GT>::BITS / 8;
    unsigned* hist = (unsigned*)ws;
    DeState* states = (DeState*)(ws + DE_STATE_OFF);
    double* fin = (double*)(ws + DE_FINAL_OFF);
    double* partials = (double*)(ws + DE_PART_OFF);
    const GT lo = (GT)dmin, hi = (GT)dmax;                                  // the bounds in the ground truth's own precision
    const int blocks = de_blocks(win.area);
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)np * DE_HIST_INTS * sizeof(unsigned), stream);
    if (e != hipSuccess) return (int)e;
    for (int p = 0; p < np; ++p)
        hipLaunchKernelGGL(de_hist_kernel<GT>, dim3(blocks), dim3(DE_THREADS), 0, stream, gt, pred, win, lo, hi, hist, states, p);
    hipLaunchKernelGGL(de_metric_kernel<GT>, dim3(blocks), dim3(DE_THREADS), 0, stream, gt, pred, win, lo, hi, dmin, dmax, hist, states, np, fin,
                       partials);
    hipLaunchKernelGGL(de_row_kernel, dim3(1), dim3(64), 0, stream, fin, partials, blocks, row);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_depth_eval_score(const void* gt, int gt_dtype, const float* pred, int H, int W, int r0, int r1, int c0, int c1,
                                     double min_depth, double max_depth, void* ws, long ws_bytes, double* rows, int row, int capacity,
                                     hipStream_t stream) {
    UENC_CHECK_ARG(gt && pred && ws && rows);
    UENC_CHECK_ARG(gt_dtype == UENC_F32 || gt_dtype == UENC_EXT_F64);
    UENC_CHECK_ARG(de_aligned(gt, gt_dtype == UENC_F32 ? 4 : 8) && de_aligned(pred, 4) && de_aligned(ws, 8) && de_aligned(rows, 8));
    UENC_CHECK_ARG(de_size_ok(H, W));
    UENC_CHECK_ARG(r0 >= 0 && r0 < r1 && r1 <= H && c0 >= 0 && c0 < c1 && c1 <= W);
    UENC_CHECK_ARG(min_depth < max_depth);                                  // false for a NaN as well
    UENC_CHECK_ARG(ws_bytes >= uenc_depth_eval_ws_bytes(H, W));
    UENC_CHECK_ARG(capacity >= 1 && row >= 0 && row < capacity);
    DeWindow win;
    win.W = W; win.r0 = r0; win.c0 = c0; win.ww = c1 - c0; win.area = (r1 - r0) * (c1 - c0);
    double* out = rows + (size_t)row * UENC_DEPTH_EVAL_ROW;
    if (gt_dtype == UENC_F32) return de_score<float>(gt, pred, win, min_depth, max_depth, (char*)ws, out, stream);
    return de_score<double>(gt, pred, win, min_depth, max_depth, (char*)ws, out, stream);
}
