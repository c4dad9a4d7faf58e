// The set criterion's hot path (uenc.modeling.criterion.SetCriterion): point-sampled mask and dice losses of the matched
// (prediction, target) pairs and the weighted class loss, for ALL prediction heads in one launch each, fp32, no float atomics.
//
// A pair is one matched (query, target) of one image of one head.  The pairs of a head run over the images in order and within an image in
// the matcher's order, N = sum_b min(Q, T_b) per head; row r = head * N + n of every buffer belongs to pair n of that head.  The query and
// target of a pair are READ from the matcher's flat device index buffers (row_ind / col_ind, heads * N entries), never from the host; a
// pair whose indices are out of range (the device solver writes -1 when it fails) is inert: zero losses, no taps.
//
//   uenc_crit_point_logits     the predicted logit map of every pair at M points (the oversampled pass of the importance sampling)
//   uenc_crit_mask_loss_fwd    one workgroup per pair: logit map and uint8 target sampled at the P final points, the four sums reduced in a
//                              fixed tree, ce_n and dice_n, and per point the two unit gradients d ce_n / d x_p, d dice_n / d x_p plus the
//                              cell index of each of its four bilinear taps (h * w = no cell) for the backward
//   uenc_crit_mask_loss_bwd    the gradient of every head's pred_masks.  The caller sorts each pair's 4 P tap keys (stable); the lane at the
//                              head of a run of equal keys adds its run serially in sorted order and writes the cell with one plain store
//                              into the zero-filled gradient: each cell is written at most once, nothing is read-modify-written
//   uenc_crit_class_loss       target classes from the indices, log-softmax, weighted NLL and its normaliser; one wave per (head, row),
//                              then one workgroup per head adds the rows in a fixed order and normalises the gradient
//
// The descriptor is a HOST block the entry points copy into the kernel arguments (as uenc_match_cost does): a stream capture records the
// pointers by value.  The bilinear taps are grid_sample(map, 2 p - 1, align_corners = False, zero padding), the arithmetic of matcher.hip.
#include "common.h"

#define CRIT_MAX_HEADS 16
#define CRIT_MAX_IMAGES 32
#define CRIT_MAX_POINTS (1 << 21)

struct CritHead {
    const float* masks;           // (bs, Q, h, w) mask logits of this head
    const float* logits;          // (bs, Q, C1) class logits
};
struct CritImage {
    const unsigned char* gt;      // (T, Hg, Wg) 0 / 1
    const long long* labels;      // (T)
    int T, pair0;                 // pair0 = sum of min(Q, T) over the images before this one
};
struct CritDesc { CritHead head[CRIT_MAX_HEADS]; CritImage img[CRIT_MAX_IMAGES]; };
static_assert(sizeof(CritDesc) == 1024, "descriptor layout is part of the ABI");

struct CTaps { int x0, y0; float wgt[4]; };               // taps nw, ne, sw, se
__device__ __forceinline__ CTaps crit_taps(float px, float py, int H, int W) {
    const float ix = ((2.f * px - 1.f + 1.f) * (float)W - 1.f) * 0.5f, iy = ((2.f * py - 1.f + 1.f) * (float)H - 1.f) * 0.5f;
    const float fx = floorf(ix), fy = floorf(iy);
    CTaps t;
    // a coordinate far outside the map (or NaN) has no tap in range: park it where every bounds test fails
    t.x0 = (fx >= -2.f && fx <= (float)W) ? (int)fx : -4;
    t.y0 = (fy >= -2.f && fy <= (float)H) ? (int)fy : -4;
    const float ex = fx + 1.f - ix, ey = fy + 1.f - iy, dx = ix - fx, dy = iy - fy;
    t.wgt[0] = ex * ey; t.wgt[1] = dx * ey; t.wgt[2] = ex * dy; t.wgt[3] = dx * dy;
    return t;
}
// cell index y * W + x of tap c, or H * W when the tap lies outside the map
__device__ __forceinline__ int crit_cell(const CTaps& t, int c, int H, int W) {
    const int x = t.x0 + (c & 1), y = t.y0 + (c >> 1);
    return (x >= 0 && x < W && y >= 0 && y < H) ? y * W + x : H * W;
}
template <typename T>
__device__ __forceinline__ float crit_sample(const T* __restrict__ map, const CTaps& t, int H, int W) {
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int cell = crit_cell(t, c, H, W);
        if (cell < H * W) v += (float)map[cell] * t.wgt[c];
    }
    return v;
}

__device__ __forceinline__ int crit_image_of(const CritDesc& d, int bs, int n) {
    int b = 0;
    while (b + 1 < bs && n >= d.img[b + 1].pair0) ++b;
    return b;
}

__global__ __launch_bounds__(256) void crit_point_logits_kernel(CritDesc d, int bs, int Q, int h, int w, int N, int M,
                                                                const long long* __restrict__ row_ind, const float* __restrict__ points,
                                                                float* __restrict__ out) {
    const long r = blockIdx.x;
    const int head = (int)(r / N), n = (int)(r % N), m = blockIdx.y * 256 + threadIdx.x;
    if (m >= M) return;
    const int b = crit_image_of(d, bs, n);
    const long long q = row_ind[r];
    float x = 0.f;
    if (q >= 0 && q < Q) {
        const float* pt = points + (r * M + m) * 2;
        x = crit_sample(d.head[head].masks + ((long)b * Q + q) * h * w, crit_taps(pt[0], pt[1], h, w), h, w);
    }
    out[r * M + m] = x;
}

// sums of four values over the 256 lanes of a workgroup in a fixed order: the xor butterfly inside each wave, then wave 0 .. 3
__device__ __forceinline__ void crit_block_sum4(float (&v)[4], float (*red)[4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = wave_sum(v[i]);
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[wave][i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

__global__ __launch_bounds__(256) void crit_mask_loss_fwd_kernel(CritDesc d, int bs, int Q, int h, int w, int Hg, int Wg, int N, int P,
                                                                 const long long* __restrict__ row_ind, const long long* __restrict__ col_ind,
                                                                 const float* __restrict__ points, float* __restrict__ loss,
                                                                 float* __restrict__ sums, float* __restrict__ unit, int* __restrict__ keys) {
    __shared__ float red[4][4];
    const long r = blockIdx.x;
    const int head = (int)(r / N), n = (int)(r % N), tid = threadIdx.x;
    const int b = crit_image_of(d, bs, n);
    const long long q = row_ind[r], t = col_ind[r];
    const bool valid = q >= 0 && q < Q && t >= 0 && t < d.img[b].T;
    const float* xmap = d.head[head].masks + ((long)b * Q + (valid ? q : 0)) * h * w;
    const unsigned char* tmap = d.img[b].gt + (long)(valid ? t : 0) * Hg * Wg;
    const float* pts = points + r * P * 2;
    float* un = unit ? unit + r * P * 2 : nullptr;
    int* ky = keys ? keys + r * P * 4 : nullptr;

    float acc[4] = {0.f, 0.f, 0.f, 0.f};                  // sum bce, sum s t, sum s, sum t
    for (int p = tid; p < P; p += 256) {
        float s = 0.f, tt = 0.f;
        int cell[4] = {h * w, h * w, h * w, h * w};
        if (valid) {
            const CTaps tp = crit_taps(pts[2L * p], pts[2L * p + 1], h, w);
            const float x = crit_sample(xmap, tp, h, w);
            tt = crit_sample(tmap, crit_taps(pts[2L * p], pts[2L * p + 1], Hg, Wg), Hg, Wg);
            const float e = expf(-fabsf(x)), dd = 1.f / (1.f + e);
            s = x >= 0.f ? dd : e * dd;                   // sigmoid(x)
            acc[0] += fmaxf(x, 0.f) - x * tt + log1pf(e); // binary cross entropy with logits
            acc[1] += s * tt; acc[2] += s; acc[3] += tt;
#pragma unroll
            for (int c = 0; c < 4; ++c) cell[c] = crit_cell(tp, c, h, w);
        }
        if (un) { un[2L * p] = s; un[2L * p + 1] = tt; }
        if (ky) *(int4*)(ky + 4L * p) = make_int4(cell[0], cell[1], cell[2], cell[3]);
    }
    crit_block_sum4(acc, red);
    const float D = acc[2] + acc[3] + 1.f, Nn = 2.f * acc[1] + 1.f;
    if (tid == 0) {
        loss[2 * r] = valid ? acc[0] / (float)P : 0.f;
        loss[2 * r + 1] = valid ? 1.f - Nn / D : 0.f;
        sums[3 * r] = acc[1]; sums[3 * r + 1] = acc[2]; sums[3 * r + 2] = acc[3];
    }
    if (!un) return;
    // second pass, each lane over the points it wrote: s, t -> d ce_n / d x_p = (s - t) / P and d dice_n / d x_p
    const float invP = 1.f / (float)P, invD2 = 1.f / (D * D);
    for (int p = tid; p < P; p += 256) {
        const float s = un[2L * p], tt = un[2L * p + 1];
        un[2L * p] = valid ? (s - tt) * invP : 0.f;
        un[2L * p + 1] = valid ? -(2.f * tt * D - Nn) * invD2 * (s * (1.f - s)) : 0.f;
    }
}

__global__ __launch_bounds__(256) void crit_mask_loss_bwd_kernel(CritDesc d, int bs, int Q, int h, int w, int N, int P,
                                                                 const long long* __restrict__ row_ind, const float* __restrict__ points,
                                                                 const float* __restrict__ unit, const int* __restrict__ skeys,
                                                                 const long long* __restrict__ order, const float* __restrict__ gce,
                                                                 const float* __restrict__ gdice, float inv_num_masks, float* __restrict__ gmasks) {
    const long r = blockIdx.x;
    const int head = (int)(r / N), n = (int)(r % N), j = blockIdx.y * 256 + threadIdx.x, P4 = 4 * P;
    if (j >= P4) return;
    const int* sk = skeys + r * P4;
    const int key = sk[j];
    if (key < 0 || key >= h * w) return;                  // a tap outside the map
    if (j > 0 && sk[j - 1] == key) return;                // not the head of its run
    const long long q = row_ind[r];
    if (q < 0 || q >= Q) return;
    const int b = crit_image_of(d, bs, n);
    const long long* od = order + r * P4;
    const float* pts = points + r * P * 2;
    const float* un = unit + r * P * 2;
    const float ca = gce[head] * inv_num_masks, cd = gdice[head] * inv_num_masks;
    float sum = 0.f;
    for (int k = j; k < P4 && sk[k] == key; ++k) {
        const long long tap = od[k];
        if (tap < 0 || tap >= P4) continue;
        const int p = (int)(tap >> 2), c = (int)(tap & 3);
        const CTaps tp = crit_taps(pts[2L * p], pts[2L * p + 1], h, w);
        const float wt = c == 0 ? tp.wgt[0] : c == 1 ? tp.wgt[1] : c == 2 ? tp.wgt[2] : tp.wgt[3];
        sum += wt * (ca * un[2L * p] + cd * un[2L * p + 1]);
    }
    gmasks[(((long)head * bs + b) * Q + q) * h * w + key] = sum;
}

__global__ __launch_bounds__(64) void crit_class_rows_kernel(CritDesc d, int bs, int Q, int C1, int N, const long long* __restrict__ row_ind,
                                                             const long long* __restrict__ col_ind, float eos_coef, float* __restrict__ rows,
                                                             float* __restrict__ grad) {
    const int row = blockIdx.x, head = blockIdx.y, lane = threadIdx.x;
    const int b = row / Q, q = row % Q, T = d.img[b].T;
    const int cnt = Q < T ? Q : T;
    const long base = (long)head * N + d.img[b].pair0;
    int k = 0x7fffffff;                                   // the first pair of this image whose query is q
    for (int i = lane; i < cnt; i += 64)
        if (row_ind[base + i] == q) { k = i; break; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k = min(k, __shfl_xor(k, o));
    long long y = C1 - 1;                                 // no-object
    if (k != 0x7fffffff) {
        const long long t = col_ind[base + k];
        y = (t >= 0 && t < T) ? d.img[b].labels[t] : -1;
    }
    const bool ok = y >= 0 && y < C1;                     // a label outside [0, C1) takes the row out of the loss
    const float wgt = !ok ? 0.f : (y == C1 - 1 ? eos_coef : 1.f);
    const float* lg = d.head[head].logits + (long)row * C1;
    float m = -__builtin_inff();
    for (int c = lane; c < C1; c += 64) m = fmaxf(m, lg[c]);
    m = wave_max(m);
    float se = 0.f;
    for (int c = lane; c < C1; c += 64) se += expf(lg[c] - m);
    se = wave_sum(se);
    const float lse = m + logf(se);
    const long ro = (long)head * bs * Q + row;
    float* g = grad + ro * C1;
    for (int c = lane; c < C1; c += 64) g[c] = ok ? wgt * (expf(lg[c] - lse) - (c == y ? 1.f : 0.f)) : 0.f;
    if (lane == 0) {
        rows[2 * ro] = ok ? wgt * (lse - lg[y]) : 0.f;
        rows[2 * ro + 1] = wgt;
    }
}

__global__ __launch_bounds__(256) void crit_class_finish_kernel(int R, int C1, const float* __restrict__ rows, float* __restrict__ loss,
                                                                float* __restrict__ grad) {
    __shared__ double red[2][4];
    const int head = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* rw = rows + 2L * head * R;
    double a = 0.0, bsum = 0.0;
    for (int i = tid; i < R; i += 256) { a += (double)rw[2 * i]; bsum += (double)rw[2 * i + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); bsum += __shfl_xor(bsum, o); }
    if (lane == 0) { red[0][wave] = a; red[1][wave] = bsum; }
    __syncthreads();
    a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    bsum = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    if (tid == 0) loss[head] = (float)(a / bsum);
    const float inv = (float)(1.0 / bsum);
    float* g = grad + (long)head * R * C1;
    for (long e = tid; e < (long)R * C1; e += 256) g[e] *= inv;
}

// the shape of a call and its descriptor: every pointer the kernels follow, and pair0 = the running sum of min(Q, T)
static bool crit_desc_ok(const CritDesc* d, int n_heads, int bs, int Q, int N, bool need_masks, bool need_logits, bool need_gt) {
    if (d == nullptr || n_heads < 1 || n_heads > CRIT_MAX_HEADS || bs < 1 || bs > CRIT_MAX_IMAGES || Q < 1 || Q > 256 || N < 0) return false;
    for (int i = 0; i < n_heads; ++i) {
        if (need_masks && (d->head[i].masks == nullptr || (((uintptr_t)d->head[i].masks) & 3) != 0)) return false;
        if (need_logits && (d->head[i].logits == nullptr || (((uintptr_t)d->head[i].logits) & 3) != 0)) return false;
    }
    int pairs = 0;
    for (int b = 0; b < bs; ++b) {
        const CritImage& im = d->img[b];
        if (im.T < 0 || im.T > 256 || im.pair0 != pairs) return false;
        if (im.T > 0 && need_gt && (im.gt == nullptr || im.labels == nullptr || (((uintptr_t)im.labels) & 7) != 0)) return false;
        pairs += Q < im.T ? Q : im.T;
    }
    return pairs == N;
}
static inline bool crit_map_ok(int h, int w) { return h >= 1 && w >= 1 && h <= 16384 && w <= 16384; }
static inline unsigned crit_chunks(int n) { return (unsigned)((n + 255) / 256); }

extern "C" int uenc_crit_point_logits(const void* desc, int n_heads, int bs, int Q, int h, int w, int N, int M, const long long* row_ind,
                                      const float* points, float* out, hipStream_t stream) {
    UENC_CHECK_ARG(crit_desc_ok((const CritDesc*)desc, n_heads, bs, Q, N, true, false, false) && crit_map_ok(h, w));
    UENC_CHECK_ARG(N >= 1 && M >= 1 && M <= CRIT_MAX_POINTS && row_ind != nullptr && points != nullptr && out != nullptr);
    UENC_CHECK_ARG((((uintptr_t)row_ind) & 7) == 0 && (((uintptr_t)points | (uintptr_t)out) & 3) == 0);
    hipLaunchKernelGGL(crit_point_logits_kernel, dim3((unsigned)n_heads * N, crit_chunks(M)), dim3(256), 0, stream, *(const CritDesc*)desc, bs, Q,
                       h, w, N, M, row_ind, points, out);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_crit_mask_loss_fwd(const void* desc, int n_heads, int bs, int Q, int h, int w, int Hg, int Wg, int N, int P,
                                       const long long* row_ind, const long long* col_ind, const float* points, float* loss, float* sums,
                                       float* unit, int* keys, hipStream_t stream) {
    UENC_CHECK_ARG(crit_desc_ok((const CritDesc*)desc, n_heads, bs, Q, N, true, false, true) && crit_map_ok(h, w) && crit_map_ok(Hg, Wg));
    UENC_CHECK_ARG(N >= 1 && P >= 1 && P <= CRIT_MAX_POINTS && row_ind != nullptr && col_ind != nullptr && points != nullptr && loss != nullptr && sums != nullptr);
    UENC_CHECK_ARG((unit == nullptr) == (keys == nullptr));
    UENC_CHECK_ARG((((uintptr_t)row_ind | (uintptr_t)col_ind) & 7) == 0 && (((uintptr_t)points | (uintptr_t)loss | (uintptr_t)sums | (uintptr_t)unit) & 3) == 0);
    UENC_CHECK_ARG((((uintptr_t)keys) & 15) == 0);
    hipLaunchKernelGGL(crit_mask_loss_fwd_kernel, dim3((unsigned)n_heads * N), dim3(256), 0, stream, *(const CritDesc*)desc, bs, Q, h, w, Hg, Wg, N,
                       P, row_ind, col_ind, points, loss, sums, unit, keys);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_crit_mask_loss_bwd(const void* desc, int n_heads, int bs, int Q, int h, int w, int N, int P, const long long* row_ind,
                                       const float* points, const float* unit, const int* sorted_keys, const long long* order, const float* gce,
                                       const float* gdice, float inv_num_masks, float* gmasks, hipStream_t stream) {
    UENC_CHECK_ARG(crit_desc_ok((const CritDesc*)desc, n_heads, bs, Q, N, false, false, false) && crit_map_ok(h, w));
    UENC_CHECK_ARG(N >= 1 && P >= 1 && P <= CRIT_MAX_POINTS && row_ind != nullptr && points != nullptr && unit != nullptr && sorted_keys != nullptr);
    UENC_CHECK_ARG(order != nullptr && gce != nullptr && gdice != nullptr && gmasks != nullptr);
    UENC_CHECK_ARG((((uintptr_t)row_ind | (uintptr_t)order) & 7) == 0);
    UENC_CHECK_ARG((((uintptr_t)points | (uintptr_t)unit | (uintptr_t)sorted_keys | (uintptr_t)gce | (uintptr_t)gdice | (uintptr_t)gmasks) & 3) == 0);
    hipLaunchKernelGGL(crit_mask_loss_bwd_kernel, dim3((unsigned)n_heads * N, crit_chunks(4 * P)), dim3(256), 0, stream, *(const CritDesc*)desc, bs,
                       Q, h, w, N, P, row_ind, points, unit, sorted_keys, order, gce, gdice, inv_num_masks, gmasks);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_crit_class_loss(const void* desc, int n_heads, int bs, int Q, int C1, int N, const long long* row_ind, const long long* col_ind,
                                    float eos_coef, float* rows, float* loss, float* grad, hipStream_t stream) {
    // N may be 0 here: a batch without targets still has a class loss (every query is no-object)
    UENC_CHECK_ARG(crit_desc_ok((const CritDesc*)desc, n_heads, bs, Q, N, false, true, true));
    UENC_CHECK_ARG(C1 >= 2 && C1 <= 65536 && rows != nullptr && loss != nullptr && grad != nullptr && (N == 0 || (row_ind != nullptr && col_ind != nullptr)));
    UENC_CHECK_ARG((((uintptr_t)row_ind | (uintptr_t)col_ind) & 7) == 0 && (((uintptr_t)rows | (uintptr_t)loss | (uintptr_t)grad) & 3) == 0);
    hipLaunchKernelGGL(crit_class_rows_kernel, dim3((unsigned)bs * Q, n_heads), dim3(64), 0, stream, *(const CritDesc*)desc, bs, Q, C1, N, row_ind, col_ind, eos_coef,
                       rows, grad);
    hipLaunchKernelGGL(crit_class_finish_kernel, dim3(n_heads), dim3(256), 0, stream, bs * Q, C1, (const float*)rows, loss, grad);
    UENC_LAUNCH_RET();
}
