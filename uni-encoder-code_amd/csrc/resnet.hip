// ResNet backbone kernels (uenc/modeling/backbone/resnet.py): the patch gather of the 7x7 stride-2 stem, the 3x3 stride-2 max pooling
// and BatchNorm (train / eval / frozen) with the residual add and the ReLU that follow it in every block.
//
// All maps are channels-last; a thread owns 8 consecutive channels of one pixel (one 16-byte bf16 or two 16-byte fp32 accesses), so
// C % 8 == 0 throughout.  Per-channel reductions over the rows of an (M, C) matrix (batch statistics, dgamma / dbeta) are done in
// two launches without atomics: every workgroup reduces one row slab and STORES its partial to a workspace slab, a second small
// kernel combines the slabs in a fixed order -- the same inputs give the same bits.  Batch statistics are Welford accumulations per
// thread combined by Chan's pairwise update (in LDS across the threads of a workgroup, then across the slabs): no E[x^2] - E[x]^2.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kReduceSlabs = 1024;      // slabs of a reduction: its second pass walks them one by one
constexpr int kMapSlabs = 16384;        // row slabs of an elementwise pass

__device__ __forceinline__ void ld8(const void* p, int dtype, long off, float v[8]) {
    if (dtype == UENC_BF16) {
        const bf16x8 r = *(const bf16x8*)((const bf16*)p + off);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)r[j];
    } else {
        const float4 a = *(const float4*)((const float*)p + off), b = *(const float4*)((const float*)p + off + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
}
__device__ __forceinline__ void st8(void* p, int dtype, long off, const float v[8]) {
    if (dtype == UENC_BF16) {
        bf16x8 r;
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = (bf16)v[j];
        *(bf16x8*)((bf16*)p + off) = r;
    } else {
        *(float4*)((float*)p + off) = make_float4(v[0], v[1], v[2], v[3]);
        *(float4*)((float*)p + off + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
}

// ---- stem: patch matrix of the 7x7 stride-2 padding-3 convolution on the 3-channel NCHW image ------------------------------------
// One thread writes 8 consecutive columns (16 bytes of bf16 / 32 of fp32) of one row; column j < 147 is tap (ky, kx, c) = (j / 21,
// (j / 3) % 7, j % 3), columns 147..151 are zero.
constexpr int kStemK = 147, kStemKp = 152;

__global__ __launch_bounds__(kThreads) void stem_patches_kernel(const float* __restrict__ x, void* __restrict__ col, int col_dtype, int B, int H,
                                                                int W, int Ho, int Wo) {
    const long total = (long)B * Ho * Wo * (kStemKp / 8);
    for (long t = (long)blockIdx.x * kThreads + threadIdx.x; t < total; t += (long)gridDim.x * kThreads) {
        const int j8 = (int)(t % (kStemKp / 8));
        long r = t / (kStemKp / 8);
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const int b = (int)(r / Ho);
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = j8 * 8 + i;
            const int ky = j / 21, kx = (j / 3) % 7, c = j % 3;
            const int iy = 2 * oy + ky - 3, ix = 2 * ox + kx - 3;
            const bool in = j < kStemK && iy >= 0 && iy < H && ix >= 0 && ix < W;
            v[i] = in ? x[(((long)b * 3 + c) * H + iy) * W + ix] : 0.f;
        }
        st8(col, col_dtype, t * 8, v);
    }
}

// ---- max pooling 3x3 stride 2 padding 1 ------------------------------------------------------------------------------------------
// Padding never wins (the running maximum starts at -inf on the first tap inside the map); a later tap replaces the maximum only when
// it is greater (or NaN), so ties keep the first maximum in (ky, kx) scan order, which is what ATen selects and routes the gradient to.
// The selected tap (ky * 3 + kx) is saved as one byte per output element for the backward.
__global__ __launch_bounds__(kThreads) void maxpool_fwd_kernel(const void* __restrict__ x, void* __restrict__ y, uint8_t* __restrict__ idx, int dtype,
                                                               int B, int H, int W, int C, int Ho, int Wo) {
    const int c8n = C >> 3;
    const long total = (long)B * Ho * Wo * c8n;
    for (long t = (long)blockIdx.x * kThreads + threadIdx.x; t < total; t += (long)gridDim.x * kThreads) {
        const int c8 = (int)(t % c8n);
        long r = t / c8n;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const int b = (int)(r / Ho);
        float best[8];
        int sel[8];
        const int ky0 = oy == 0 ? 1 : 0, kx0 = ox == 0 ? 1 : 0;               // first tap inside the map
#pragma unroll
        for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; sel[j] = ky0 * 3 + kx0; }
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy + ky - 1;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox + kx - 1;
                if (ix < 0 || ix >= W) continue;
                float v[8];
                ld8(x, dtype, (((long)b * H + iy) * W + ix) * C + c8 * 8, v);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (v[j] > best[j] || v[j] != v[j]) { best[j] = v[j]; sel[j] = ky * 3 + kx; }
            }
        }
        st8(y, dtype, t * 8, best);
        u32x2 packed;
        packed[0] = (unsigned)sel[0] | ((unsigned)sel[1] << 8) | ((unsigned)sel[2] << 16) | ((unsigned)sel[3] << 24);
        packed[1] = (unsigned)sel[4] | ((unsigned)sel[5] << 8) | ((unsigned)sel[6] << 16) | ((unsigned)sel[7] << 24);
        *(u32x2*)(idx + t * 8) = packed;
    }
}

// Gather form: an input element lies in at most 2 x 2 windows; it adds the gradient of those whose saved tap is its own.
__global__ __launch_bounds__(kThreads) void maxpool_bwd_kernel(const void* __restrict__ dy, const uint8_t* __restrict__ idx, void* __restrict__ dx,
                                                               int dtype, int B, int H, int W, int C, int Ho, int Wo) {
    const int c8n = C >> 3;
    const long total = (long)B * H * W * c8n;
    for (long t = (long)blockIdx.x * kThreads + threadIdx.x; t < total; t += (long)gridDim.x * kThreads) {
        const int c8 = (int)(t % c8n);
        long r = t / c8n;
        const int ix = (int)(r % W); r /= W;
        const int iy = (int)(r % H);
        const int b = (int)(r / H);
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // windows oy with 2 oy - 1 <= iy <= 2 oy + 1: oy = iy / 2 for an even row (tap 1), (iy - 1) / 2 (tap 2) and (iy + 1) / 2 (tap 0) for an odd one
        const int oy_lo = iy >> 1, oy_hi = (iy + 1) >> 1, ox_lo = ix >> 1, ox_hi = (ix + 1) >> 1;
        for (int oy = oy_lo; oy <= oy_hi; ++oy) {
            if (oy >= Ho) continue;
            const int ky = iy - (2 * oy - 1);
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                if (ox >= Wo) continue;
                const int kx = ix - (2 * ox - 1);
                const long o = (((long)b * Ho + oy) * Wo + ox) * C + c8 * 8;
                const u32x2 packed = *(const u32x2*)(idx + o);
                float g[8];
                ld8(dy, dtype, o, g);
                const unsigned mine = (unsigned)(ky * 3 + kx);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (((packed[j >> 2] >> (8 * (j & 3))) & 0xffu) == mine) acc[j] += g[j];
            }
        }
        st8(dx, dtype, t * 8, acc);
    }
}

// ---- per-channel reductions over the rows of (M, C) -----------------------------------------------------------------------------
// Tiling shared by the reduction and the elementwise BatchNorm kernels: a workgroup covers CT = min(C / 8, 32) channel chunks
// (blockIdx.y picks the tile) and RL = 256 / CT row lanes; a thread keeps its 8 channels and walks the rows of its slab
// (blockIdx.x) with stride RL, so per-channel values (scale, shift, statistics) are loaded once per thread.
struct Tiling {
    int ct, rl, tiles, slabs;
    long rows_per_slab;
};
static Tiling make_tiling(long M, int C, int max_slabs, int min_rows) {
    Tiling t;
    const int c8n = C / 8;
    t.ct = c8n < 32 ? c8n : 32;
    t.rl = kThreads / t.ct;
    t.tiles = (c8n + t.ct - 1) / t.ct;
    long slabs = ceil_div64(M, (long)t.rl * min_rows);             // at least min_rows rows per thread before another slab is opened
    const long cap = max_slabs / t.tiles > 0 ? max_slabs / t.tiles : 1;
    if (slabs > cap) slabs = cap;
    if (slabs < 1) slabs = 1;
    t.rows_per_slab = ceil_div64(M, slabs);
    t.slabs = (int)ceil_div64(M, t.rows_per_slab);
    return t;
}

static Tiling reduce_tiling(long M, int C) { return make_tiling(M, C, kReduceSlabs, 8); }
static Tiling map_tiling(long M, int C) { return make_tiling(M, C, kMapSlabs, 4); }

// LDS tree over the row lanes of a workgroup: thread t keeps 16 floats, value j at sm[j * 256 + t] (for a fixed j the lanes of a wave read
// consecutive words, partner t + s * CT included: no bank conflicts).  Stride s runs over powers of two from the one at or
// above RL / 2 downwards; lanes without a partner keep their value.
__device__ __forceinline__ int tree_start(int rl) {
    int s = 1;
    while (s * 2 < rl) s *= 2;
    return rl > 1 ? s : 0;
}

// Welford over a thread's rows, then Chan merges.  part: (slabs, 2, C) = (mean, M2) per slab; the count of a slab follows from M.
__global__ __launch_bounds__(kThreads) void bn_stats_partial_kernel(const void* __restrict__ x, int dtype, long M, int C, int CT, int RL,
                                                                    long rows_per_slab, float* __restrict__ part) {
    __shared__ float sm[kThreads * 16];
    __shared__ float sn[kThreads];
    const int cl = threadIdx.x % CT, rl = threadIdx.x / CT;
    const int c8 = blockIdx.y * CT + cl;
    const bool live = rl < RL && c8 * 8 < C;
    const long r0 = (long)blockIdx.x * rows_per_slab;
    const long r1 = r0 + rows_per_slab < M ? r0 + rows_per_slab : M;
    float mean[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, m2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float n = 0.f;
    if (live) {
        for (long r = r0 + rl; r < r1; r += RL) {
            float v[8];
            ld8(x, dtype, r * C + c8 * 8, v);
            n += 1.f;
            const float inv = 1.f / n;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[j] - mean[j];
                mean[j] += d * inv;
                m2[j] += d * (v[j] - mean[j]);
            }
        }
    }
    float* e = sm + threadIdx.x;                    // value j of this thread at e[j * kThreads]: a wave's lanes touch consecutive banks
#pragma unroll
    for (int j = 0; j < 8; ++j) { e[j * kThreads] = mean[j]; e[(8 + j) * kThreads] = m2[j]; }
    sn[threadIdx.x] = n;
    __syncthreads();
    for (int s = tree_start(RL); s > 0; s >>= 1) {
        if (live && rl < s && rl + s < RL) {
            const float* o = sm + threadIdx.x + s * CT;
            const float nb = sn[threadIdx.x + s * CT], na = sn[threadIdx.x];
            if (nb > 0.f) {
                const float nt = na + nb, fb = nb / nt;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float d = o[j * kThreads] - e[j * kThreads];
                    e[(8 + j) * kThreads] += o[(8 + j) * kThreads] + d * d * na * fb;
                    e[j * kThreads] += d * fb;
                }
                sn[threadIdx.x] = nt;
            }
        }
        __syncthreads();
    }
    if (live && rl == 0) {
        float* p = part + (long)blockIdx.x * 2 * C + c8 * 8;
        *(float4*)p = make_float4(e[0 * kThreads], e[1 * kThreads], e[2 * kThreads], e[3 * kThreads]);
        *(float4*)(p + 4) = make_float4(e[4 * kThreads], e[5 * kThreads], e[6 * kThreads], e[7 * kThreads]);
        *(float4*)(p + C) = make_float4(e[8 * kThreads], e[9 * kThreads], e[10 * kThreads], e[11 * kThreads]);
        *(float4*)(p + C + 4) = make_float4(e[12 * kThreads], e[13 * kThreads], e[14 * kThreads], e[15 * kThreads]);
    }
}

// One thread per channel merges the slabs in order, writes mean and biased variance, and updates the running statistics
// (unbiased variance) and the batch counter.
__global__ __launch_bounds__(kThreads) void bn_stats_finish_kernel(const float* __restrict__ part, int slabs, long rows_per_slab, long M, int C,
                                                                   float* __restrict__ mean, float* __restrict__ var, float* running_mean,
                                                                   float* running_var, long long* num_batches_tracked, float momentum) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c == 0 && num_batches_tracked) num_batches_tracked[0] += 1;
    if (c >= C) return;
    float na = 0.f, mu = 0.f, m2 = 0.f;
    for (int s = 0; s < slabs; ++s) {
        const long r0 = (long)s * rows_per_slab;
        const float nb = (float)((r0 + rows_per_slab < M ? r0 + rows_per_slab : M) - r0);
        const float mb = part[(long)s * 2 * C + c], vb = part[(long)s * 2 * C + C + c];
        const float nt = na + nb, fb = nb / nt, d = mb - mu;
        m2 += vb + d * d * na * fb;
        mu += d * fb;
        na = nt;
    }
    const float v = m2 / (float)M;
    mean[c] = mu;
    var[c] = v;
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
    if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (m2 / (float)(M - 1));
}

// y = act(x * s[c] + t[c] (+ res)),  s = gamma * rsqrt(var + eps),  t = beta - mean * s  (gamma / beta NULL: 1 / 0).
__global__ __launch_bounds__(kThreads) void bn_act_fwd_kernel(const void* __restrict__ x, int x_dtype, const float* __restrict__ mean,
                                                              const float* __restrict__ var, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const void* __restrict__ res, int res_dtype,
                                                              void* __restrict__ y, int y_dtype, long M, int C, int CT, int RL, long rows_per_slab,
                                                              float eps, int relu) {
    const int cl = threadIdx.x % CT, rl = threadIdx.x / CT;
    const int c8 = blockIdx.y * CT + cl;
    if (rl >= RL || c8 * 8 >= C) return;
    float s[8], t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c8 * 8 + j;
        s[j] = (gamma ? gamma[c] : 1.f) / sqrtf(var[c] + eps);
        t[j] = (beta ? beta[c] : 0.f) - mean[c] * s[j];
    }
    const long r0 = (long)blockIdx.x * rows_per_slab;
    const long r1 = r0 + rows_per_slab < M ? r0 + rows_per_slab : M;
    for (long r = r0 + rl; r < r1; r += RL) {
        const long off = r * C + c8 * 8;
        float v[8];
        ld8(x, x_dtype, off, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] * s[j] + t[j];
        if (res) {
            float q[8];
            ld8(res, res_dtype, off, q);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += q[j];
        }
        if (relu) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] > 0.f ? v[j] : 0.f;
        }
        st8(y, y_dtype, off, v);
    }
}

// Slab partials of sum g and sum g * xhat per channel, g = dy masked by y > 0 when the node ends in a ReLU.  part: (slabs, 2, C).
__global__ __launch_bounds__(kThreads) void bn_bwd_partial_kernel(const void* __restrict__ dy, int dy_dtype, const void* __restrict__ y, int y_dtype,
                                                                  const void* __restrict__ x, int x_dtype, const float* __restrict__ mean,
                                                                  const float* __restrict__ var, long M, int C, int CT, int RL, long rows_per_slab,
                                                                  float eps, int relu, float* __restrict__ part) {
    __shared__ float sm[kThreads * 16];
    const int cl = threadIdx.x % CT, rl = threadIdx.x / CT;
    const int c8 = blockIdx.y * CT + cl;
    const bool live = rl < RL && c8 * 8 < C;
    float sg[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sgx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
        float mu[8], rstd[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            mu[j] = mean[c8 * 8 + j];
            rstd[j] = 1.f / sqrtf(var[c8 * 8 + j] + eps);
        }
        const long r0 = (long)blockIdx.x * rows_per_slab;
        const long r1 = r0 + rows_per_slab < M ? r0 + rows_per_slab : M;
        for (long r = r0 + rl; r < r1; r += RL) {
            const long off = r * C + c8 * 8;
            float g[8], v[8];
            ld8(dy, dy_dtype, off, g);
            ld8(x, x_dtype, off, v);
            if (relu) {
                float o[8];
                ld8(y, y_dtype, off, o);
#pragma unroll
                for (int j = 0; j < 8; ++j) g[j] = o[j] > 0.f ? g[j] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                sg[j] += g[j];
                sgx[j] += g[j] * ((v[j] - mu[j]) * rstd[j]);
            }
        }
    }
    float* e = sm + threadIdx.x;                    // value j of this thread at e[j * kThreads]: a wave's lanes touch consecutive banks
#pragma unroll
    for (int j = 0; j < 8; ++j) { e[j * kThreads] = sg[j]; e[(8 + j) * kThreads] = sgx[j]; }
    __syncthreads();
    for (int s = tree_start(RL); s > 0; s >>= 1) {
        if (live && rl < s && rl + s < RL) {
            const float* o = sm + threadIdx.x + s * CT;
#pragma unroll
            for (int j = 0; j < 16; ++j) e[j * kThreads] += o[j * kThreads];
        }
        __syncthreads();
    }
    if (live && rl == 0) {
        float* p = part + (long)blockIdx.x * 2 * C + c8 * 8;
        *(float4*)p = make_float4(e[0 * kThreads], e[1 * kThreads], e[2 * kThreads], e[3 * kThreads]);
        *(float4*)(p + 4) = make_float4(e[4 * kThreads], e[5 * kThreads], e[6 * kThreads], e[7 * kThreads]);
        *(float4*)(p + C) = make_float4(e[8 * kThreads], e[9 * kThreads], e[10 * kThreads], e[11 * kThreads]);
        *(float4*)(p + C + 4) = make_float4(e[12 * kThreads], e[13 * kThreads], e[14 * kThreads], e[15 * kThreads]);
    }
}

// sums (2, C) = the slabs added in order; dbeta += sums[0], dgamma += sums[1] where given.
__global__ __launch_bounds__(kThreads) void bn_bwd_finish_kernel(const float* __restrict__ part, int slabs, int C, float* __restrict__ sums,
                                                                 float* dgamma, float* dbeta) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    float a = 0.f, b = 0.f;
    for (int s = 0; s < slabs; ++s) {
        a += part[(long)s * 2 * C + c];
        b += part[(long)s * 2 * C + C + c];
    }
    sums[c] = a;
    sums[C + c] = b;
    if (dbeta) dbeta[c] += a;
    if (dgamma) dgamma[c] += b;
}

// train: dx = gamma * rstd * (g - sum_g / M - xhat * sum_gx / M);  eval / frozen: dx = g * gamma * rstd.  dres = g (the masked gradient).
__global__ __launch_bounds__(kThreads) void bn_bwd_apply_kernel(const void* __restrict__ dy, int dy_dtype, const void* __restrict__ y, int y_dtype,
                                                                const void* __restrict__ x, int x_dtype, const float* __restrict__ mean,
                                                                const float* __restrict__ var, const float* __restrict__ gamma,
                                                                const float* __restrict__ sums, void* __restrict__ dx, int dx_dtype,
                                                                void* __restrict__ dres, int dres_dtype, long M, int C, int CT, int RL,
                                                                long rows_per_slab, float eps, int relu, int train) {
    const int cl = threadIdx.x % CT, rl = threadIdx.x / CT;
    const int c8 = blockIdx.y * CT + cl;
    if (rl >= RL || c8 * 8 >= C) return;
    float mu[8], rstd[8], k[8], mg[8], mgx[8];
    const float invM = 1.f / (float)M;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c8 * 8 + j;
        mu[j] = mean[c];
        rstd[j] = 1.f / sqrtf(var[c] + eps);
        k[j] = (gamma ? gamma[c] : 1.f) * rstd[j];
        mg[j] = train ? sums[c] * invM : 0.f;
        mgx[j] = train ? sums[C + c] * invM : 0.f;
    }
    const long r0 = (long)blockIdx.x * rows_per_slab;
    const long r1 = r0 + rows_per_slab < M ? r0 + rows_per_slab : M;
    for (long r = r0 + rl; r < r1; r += RL) {
        const long off = r * C + c8 * 8;
        float g[8], o[8];
        ld8(dy, dy_dtype, off, g);
        if (relu) {
            float q[8];
            ld8(y, y_dtype, off, q);
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = q[j] > 0.f ? g[j] : 0.f;
        }
        if (train) {
            float v[8];
            ld8(x, x_dtype, off, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = k[j] * (g[j] - mg[j] - (v[j] - mu[j]) * rstd[j] * mgx[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = g[j] * k[j];
        }
        st8(dx, dx_dtype, off, o);
        if (dres) st8(dres, dres_dtype, off, g);
    }
}

inline bool dtype_ok(int d) { return d == UENC_F32 || d == UENC_BF16; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline unsigned flat_blocks(long total) {
    long blocks = (total + kThreads - 1) / kThreads;
    return (unsigned)(blocks > 65536 ? 65536 : blocks);
}

}  // namespace

extern "C" int uenc_stem7x7_s2_patches(const float* x, void* col, int col_dtype, int B, int H, int W, hipStream_t stream) {
    UENC_CHECK_ARG(x && col && dtype_ok(col_dtype) && B > 0 && H > 0 && W > 0 && aligned16(col));
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long total = (long)B * Ho * Wo * (kStemKp / 8);
    hipLaunchKernelGGL(stem_patches_kernel, dim3(flat_blocks(total)), dim3(kThreads), 0, stream, x, col, col_dtype, B, H, W, Ho, Wo);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_maxpool3x3_s2_fwd(const void* x, void* y, void* idx, int dtype, int B, int H, int W, int C, hipStream_t stream) {
    UENC_CHECK_ARG(x && y && idx && dtype_ok(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && aligned16(x) && aligned16(y) &&
                   ((uintptr_t)idx & 7) == 0);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long total = (long)B * Ho * Wo * (C / 8);
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(flat_blocks(total)), dim3(kThreads), 0, stream, x, y, (uint8_t*)idx, dtype, B, H, W, C, Ho, Wo);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_maxpool3x3_s2_bwd(const void* dy, const void* idx, void* dx, int dtype, int B, int H, int W, int C, hipStream_t stream) {
    UENC_CHECK_ARG(dy && idx && dx && dtype_ok(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && aligned16(dy) && aligned16(dx) &&
                   ((uintptr_t)idx & 7) == 0);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long total = (long)B * H * W * (C / 8);
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(flat_blocks(total)), dim3(kThreads), 0, stream, dy, (const uint8_t*)idx, dx, dtype, B, H, W, C, Ho,
                       Wo);
    UENC_LAUNCH_RET();
}

extern "C" long uenc_bn_workspace_floats(long M, int C) {
    if (M <= 0 || C <= 0 || C % 8 != 0) return -1;
    return (long)reduce_tiling(M, C).slabs * 2 * C;
}

extern "C" int uenc_bn_stats(const void* x, int x_dtype, long M, int C, float* mean, float* var, float* running_mean, float* running_var,
                             long long* num_batches_tracked, float momentum, float* workspace, long workspace_floats, hipStream_t stream) {
    UENC_CHECK_ARG(x && mean && var && workspace && dtype_ok(x_dtype) && M > 1 && C > 0 && C % 8 == 0 && aligned16(x) && aligned16(workspace));
    const Tiling t = reduce_tiling(M, C);
    UENC_CHECK_ARG(workspace_floats >= (long)t.slabs * 2 * C);
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(t.slabs, t.tiles), dim3(kThreads), 0, stream, x, x_dtype, M, C, t.ct, t.rl, t.rows_per_slab,
                       workspace);
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((C + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, (const float*)workspace, t.slabs,
                       t.rows_per_slab, M, C, mean, var, running_mean, running_var, num_batches_tracked, momentum);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_bn_act_fwd(const void* x, int x_dtype, const float* mean, const float* var, const float* gamma, const float* beta,
                               const void* res, int res_dtype, void* y, int y_dtype, long M, int C, float eps, int relu, hipStream_t stream) {
    UENC_CHECK_ARG(x && mean && var && y && dtype_ok(x_dtype) && dtype_ok(y_dtype) && (!res || dtype_ok(res_dtype)) && M > 0 && C > 0 &&
                   C % 8 == 0 && aligned16(x) && aligned16(y) && aligned16(res));
    const Tiling t = map_tiling(M, C);
    hipLaunchKernelGGL(bn_act_fwd_kernel, dim3(t.slabs, t.tiles), dim3(kThreads), 0, stream, x, x_dtype, mean, var, gamma, beta, res, res_dtype, y,
                       y_dtype, M, C, t.ct, t.rl, t.rows_per_slab, eps, relu);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_bn_act_bwd_reduce(const void* dy, int dy_dtype, const void* y, int y_dtype, const void* x, int x_dtype, const float* mean,
                                      const float* var, long M, int C, float eps, int relu, float* sums, float* dgamma, float* dbeta,
                                      float* workspace, long workspace_floats, hipStream_t stream) {
    UENC_CHECK_ARG(dy && x && mean && var && sums && workspace && (!relu || y) && dtype_ok(dy_dtype) && dtype_ok(x_dtype) &&
                   (!relu || dtype_ok(y_dtype)) && M > 0 && C > 0 && C % 8 == 0 && aligned16(dy) && aligned16(y) && aligned16(x) &&
                   aligned16(workspace));
    const Tiling t = reduce_tiling(M, C);
    UENC_CHECK_ARG(workspace_floats >= (long)t.slabs * 2 * C);
    hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(t.slabs, t.tiles), dim3(kThreads), 0, stream, dy, dy_dtype, y, y_dtype, x, x_dtype, mean, var, M,
                       C, t.ct, t.rl, t.rows_per_slab, eps, relu, workspace);
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((C + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, (const float*)workspace, t.slabs, C,
                       sums, dgamma, dbeta);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_bn_act_bwd_apply(const void* dy, int dy_dtype, const void* y, int y_dtype, const void* x, int x_dtype, const float* mean,
                                     const float* var, const float* gamma, const float* sums, void* dx, int dx_dtype, void* dres, int dres_dtype,
                                     long M, int C, float eps, int relu, int train, hipStream_t stream) {
    UENC_CHECK_ARG(dy && mean && var && dx && (!relu || y) && (!train || (x && sums)) && dtype_ok(dy_dtype) && dtype_ok(dx_dtype) &&
                   (!relu || dtype_ok(y_dtype)) && (!train || dtype_ok(x_dtype)) && (!dres || dtype_ok(dres_dtype)) && M > 0 && C > 0 &&
                   C % 8 == 0 && aligned16(dy) && aligned16(y) && aligned16(x) && aligned16(dx) && aligned16(dres));
    const Tiling t = map_tiling(M, C);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(t.slabs, t.tiles), dim3(kThreads), 0, stream, dy, dy_dtype, y, y_dtype, x, x_dtype, mean, var,
                       gamma, sums, dx, dx_dtype, dres, dres_dtype, M, C, t.ct, t.rl, t.rows_per_slab, eps, relu, train);
    UENC_LAUNCH_RET();
}
