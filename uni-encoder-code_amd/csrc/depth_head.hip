// The non-GEMM passes of the TransDSSL depth decoder in training (gfx950), each as a forward / backward pair on channels-last maps:
//   upsample2x_ac   x2 bilinear resize with align_corners=True   (reference pixel_decoder/transdssl.py: Interpolate, FeatureFusionBlock_custom)
//   softmax_gate    res = a + b, g = res * softmax_c(z)          (the attention gate of every fusion block)
//   soft_att_depth  disp = sum_k softmax(z)_k * grid_k           (SoftAttDepth)
// Operands fp32 or bf16 by the dtype tag, arithmetic in fp32, one 16-byte (bf16) or two 16-byte (fp32) accesses per 8 channels.
// No float atomics anywhere: every backward is a gather in a fixed order, so two calls give the same bits.
#include <math.h>

#include "common.h"

static bool dh_dtype(int d) { return d == UENC_F32 || d == UENC_BF16; }
static bool dh_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ void dh_ld8(const void* base, int is_f32, long idx, float* v) {
    if (is_f32) {
        const float4 a = *(const float4*)((const float*)base + idx), b = *(const float4*)((const float*)base + idx + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        const bf16x8 t = *(const bf16x8*)((const bf16*)base + idx);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)t[i];
    }
}
__device__ __forceinline__ void dh_st8(void* base, int is_f32, long idx, const float* v) {
    if (is_f32) {
        *(float4*)((float*)base + idx) = make_float4(v[0], v[1], v[2], v[3]);
        *(float4*)((float*)base + idx + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        bf16x8 t;
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = (bf16)v[i];
        *(bf16x8*)((bf16*)base + idx) = t;
    }
}

// ---- x2 bilinear upsample, align_corners=True -------------------------------------------------------------------------------------
// ATen's own arithmetic (UpSample.h: area_pixel_compute_scale / _source_index with align_corners): scale = (in - 1) / (out - 1) as an
// fp32 division (out = 2 in here, so out > 1), source = scale * dst, i0 = (int)source, i1 = i0 + (i0 < in - 1), l1 = source - i0.
__device__ __forceinline__ float up_scale(int n_in) { return (float)(n_in - 1) / (float)(2 * n_in - 1); }
__device__ __forceinline__ void up_tap(int o, float scale, int n_in, int& i0, int& i1, float& l0, float& l1) {
    const float s = scale * (float)o;
    i0 = min((int)s, n_in - 1);
    i1 = min(i0 + 1, n_in - 1);
    l1 = s - (float)i0;
    l0 = 1.0f - l1;
}

struct UpP {
    const void* src; int src_f32;       // forward: x (B, H, W, C); backward: dy (B, 2H, 2W, C)
    void* dst; int dst_f32;             // forward: y (B, 2H, 2W, C); backward: dx (B, H, W, C)
    int B, H, W, C;
};

__global__ __launch_bounds__(256) void upsample2x_ac_fwd_kernel(UpP p) {
    const int nch = p.C >> 3, Ho = 2 * p.H, Wo = 2 * p.W;
    const long total = (long)p.B * Ho * Wo * nch;
    const float sy = up_scale(p.H), sx = up_scale(p.W);
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int ck = (int)(t % nch);
        long r = t / nch;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const long b = r / Ho;
        int y0, y1, x0, x1;
        float hy0, hy1, hx0, hx1;
        up_tap(oy, sy, p.H, y0, y1, hy0, hy1);
        up_tap(ox, sx, p.W, x0, x1, hx0, hx1);
        const long row0 = (b * p.H + y0) * p.W, row1 = (b * p.H + y1) * p.W;
        float v00[8], v01[8], v10[8], v11[8], o[8];
        dh_ld8(p.src, p.src_f32, (row0 + x0) * p.C + ck * 8, v00);
        dh_ld8(p.src, p.src_f32, (row0 + x1) * p.C + ck * 8, v01);
        dh_ld8(p.src, p.src_f32, (row1 + x0) * p.C + ck * 8, v10);
        dh_ld8(p.src, p.src_f32, (row1 + x1) * p.C + ck * 8, v11);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = hy0 * (hx0 * v00[i] + hx1 * v01[i]) + hy1 * (hx0 * v10[i] + hx1 * v11[i]);
        dh_st8(p.dst, p.dst_f32, t * 8, o);
    }
}

// candidate outputs of input index i: those whose source coordinate lies in [i - 1, i + 1), one more on either side for the fp32
// rounding of the forward's product (scale > 0: n_in >= 2).  n_in == 1: both outputs read index 0.
__device__ __forceinline__ void up_range(int i, int n_in, float scale, int& lo, int& hi) {
    const int n_out = 2 * n_in;
    if (n_in == 1) { lo = 0; hi = n_out - 1; return; }
    const float inv = 1.0f / scale;
    lo = (int)floorf((float)(i - 1) * inv) - 1;
    hi = (int)ceilf((float)(i + 1) * inv) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_out - 1 ? n_out - 1 : hi;
}
// the weight output o gives input i, by the forward's own expression (both taps may be i at the clamped far edge)
__device__ __forceinline__ float up_weight(int o, float scale, int n_in, int i) {
    int i0, i1;
    float l0, l1;
    up_tap(o, scale, n_in, i0, i1, l0, l1);
    return (i0 == i ? l0 : 0.0f) + (i1 == i ? l1 : 0.0f);
}
__device__ __forceinline__ bool up_touches(int o, float scale, int n_in, int i) {
    int i0, i1;
    float l0, l1;
    up_tap(o, scale, n_in, i0, i1, l0, l1);
    return i0 == i || i1 == i;
}

// Gather form of the adjoint: input cell (i, j) adds wy * wx * dy over the outputs that touch it, oy ascending then ox ascending.
__global__ __launch_bounds__(256) void upsample2x_ac_bwd_kernel(UpP p) {
    const int nch = p.C >> 3, Wo = 2 * p.W, Ho = 2 * p.H;
    const long total = (long)p.B * p.H * p.W * nch;
    const float sy = up_scale(p.H), sx = up_scale(p.W);
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int ck = (int)(t % nch);
        long r = t / nch;
        const int j = (int)(r % p.W); r /= p.W;
        const int i = (int)(r % p.H);
        const long b = r / p.H;
        int ylo, yhi, xlo, xhi;
        up_range(i, p.H, sy, ylo, yhi);
        up_range(j, p.W, sx, xlo, xhi);
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int oy = ylo; oy <= yhi; ++oy) {
            if (!up_touches(oy, sy, p.H, i)) continue;
            const float wy = up_weight(oy, sy, p.H, i);
            for (int ox = xlo; ox <= xhi; ++ox) {
                if (!up_touches(ox, sx, p.W, j)) continue;
                const float w = wy * up_weight(ox, sx, p.W, j);
                float d[8];
                dh_ld8(p.src, p.src_f32, ((b * Ho + oy) * Wo + ox) * p.C + ck * 8, d);
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] += w * d[c];
            }
        }
        dh_st8(p.dst, p.dst_f32, t * 8, acc);
    }
}

static int up_launch(bool fwd, const void* src, int src_dtype, void* dst, int dst_dtype, int B, int H, int W, int C, hipStream_t stream) {
    UENC_CHECK_ARG(src && dst && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0);
    UENC_CHECK_ARG(dh_dtype(src_dtype) && dh_dtype(dst_dtype) && dh_aligned(src) && dh_aligned(dst));
    UENC_CHECK_ARG(H <= (1 << 20) && W <= (1 << 20));
    UpP p{src, src_dtype == UENC_F32, dst, dst_dtype == UENC_F32, B, H, W, C};
    const long total = (long)B * H * W * (C / 8) * (fwd ? 4 : 1);
    long blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    if (fwd) hipLaunchKernelGGL(upsample2x_ac_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(upsample2x_ac_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_upsample2x_ac_fwd(const void* x, int x_dtype, void* y, int y_dtype, int B, int H, int W, int C, hipStream_t stream) {
    return up_launch(true, x, x_dtype, y, y_dtype, B, H, W, C, stream);
}

extern "C" int uenc_upsample2x_ac_bwd(const void* dy, int dy_dtype, void* dx, int dx_dtype, int B, int H, int W, int C, hipStream_t stream) {
    return up_launch(false, dy, dy_dtype, dx, dx_dtype, B, H, W, C, stream);
}

// ---- row kernels: G lanes (a power of two) share one row, each lane NK pieces of 8 channels (piece gl + G * k) --------------------------
// C / 8 <= 64 pieces: NK = 1 and G the next power of two, so a 256-channel row takes half a wave and a wave two rows; wider rows take the
// whole wave with NK = 2 or 4.  The loop bounds are the same for every lane of a wave; a lane group past the last row computes on the last
// row and stores nothing.
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

struct RowP {
    const void* a; int a_f32;           // gate fwd: a            gate bwd: dg           head bwd: ddisp (fp32, per row)
    const void* b; int b_f32;           // gate fwd: b            gate bwd: d_res_in (may be NULL)
    const void* z; int z_f32;           // the logits (P, C)
    const void* res; int res_f32;       // gate bwd: res
    const float* grid;                  // head: (C) fp32
    void* o0; void* o1; int o_f32;      // gate fwd: res, g       gate bwd: d_res, d_z   head fwd: disp (fp32), -    head bwd: dz, -
    long P; int C;
};

// z becomes exp(z - max), the row's sum of them is returned (a true division by it follows, as in ATen's softmax); pieces past the
// row's end hold zeros
template <int G, int NK>
__device__ __forceinline__ float row_softmax(float (&z)[NK][8], const bool (&on)[NK]) {
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < NK; ++k)
        if (on[k]) {
#pragma unroll
            for (int i = 0; i < 8; ++i) m = fmaxf(m, z[k][i]);
        }
    m = group_max<G>(m);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            z[k][i] = on[k] ? expf(z[k][i] - m) : 0.f;
            s += z[k][i];
        }
    return group_sum<G>(s);
}

#define ROW_LOOP_BEGIN                                                                                     \
    constexpr int RPW = 64 / G;                                                                            \
    const int lane = threadIdx.x & 63, gl = lane % G, nch = p.C >> 3;                                      \
    const long nw = (long)gridDim.x * 4;                                                                   \
    bool on[NK];                                                                                           \
    _Pragma("unroll") for (int k = 0; k < NK; ++k) on[k] = gl + G * k < nch;                               \
    for (long base = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW; base < p.P; base += nw * RPW) {    \
        const long row = base + lane / G;                                                                  \
        const bool valid = row < p.P;                                                                      \
        const long off = (valid ? row : p.P - 1) * p.C + gl * 8;
#define ROW_LOOP_END }

template <int G, int NK>
__global__ __launch_bounds__(256) void softmax_gate_fwd_kernel(RowP p) {
    ROW_LOOP_BEGIN
        float z[NK][8], s[NK][8];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            if (!on[k]) continue;
            float u[8];
            dh_ld8(p.z, p.z_f32, off + G * 8 * k, z[k]);
            dh_ld8(p.a, p.a_f32, off + G * 8 * k, s[k]);
            dh_ld8(p.b, p.b_f32, off + G * 8 * k, u);
#pragma unroll
            for (int i = 0; i < 8; ++i) s[k][i] += u[i];
        }
        const float sum = row_softmax<G, NK>(z, on);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            if (!on[k] || !valid) continue;
            float g[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) g[i] = s[k][i] * (z[k][i] / sum);
            dh_st8(p.o0, p.o_f32, off + G * 8 * k, s[k]);
            dh_st8(p.o1, p.o_f32, off + G * 8 * k, g);
        }
    ROW_LOOP_END
}

template <int G, int NK>
__global__ __launch_bounds__(256) void softmax_gate_bwd_kernel(RowP p) {
    ROW_LOOP_BEGIN
        float z[NK][8], q[NK][8], dg[NK][8];           // q = dg * res
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            if (!on[k]) continue;
            dh_ld8(p.z, p.z_f32, off + G * 8 * k, z[k]);
            dh_ld8(p.res, p.res_f32, off + G * 8 * k, q[k]);
            dh_ld8(p.a, p.a_f32, off + G * 8 * k, dg[k]);
#pragma unroll
            for (int i = 0; i < 8; ++i) q[k][i] *= dg[k][i];
        }
        const float sum = row_softmax<G, NK>(z, on);
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                z[k][i] /= sum;                                                   // the attention
                dot += on[k] ? q[k][i] * z[k][i] : 0.f;
            }
        dot = group_sum<G>(dot);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            if (!on[k] || !valid) continue;
            float dr[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dz[8];
            if (p.b) dh_ld8(p.b, p.b_f32, off + G * 8 * k, dr);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                dr[i] += dg[k][i] * z[k][i];
                dz[i] = z[k][i] * (q[k][i] - dot);
            }
            dh_st8(p.o0, p.o_f32, off + G * 8 * k, dr);
            dh_st8(p.o1, p.o_f32, off + G * 8 * k, dz);
        }
    ROW_LOOP_END
}

template <int G>
__global__ __launch_bounds__(256) void soft_att_depth_kernel(RowP p, int backward) {
    constexpr int NK = 1;
    ROW_LOOP_BEGIN
        float z[1][8], gr[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (on[0]) {
            dh_ld8(p.z, p.z_f32, off, z[0]);
            dh_ld8(p.grid, 1, gl * 8, gr);
        }
        const float sum = row_softmax<G, 1>(z, on);
        float e = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            z[0][i] /= sum;
            e += z[0][i] * gr[i];
        }
        const float disp = group_sum<G>(e);
        if (!valid) continue;
        if (!backward) {
            if (gl == 0) ((float*)p.o0)[row] = disp;
        } else if (on[0]) {
            const float dd = ((const float*)p.a)[row];
            float dz[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) dz[i] = z[0][i] * (gr[i] - disp) * dd;
            dh_st8(p.o0, p.o_f32, off, dz);
        }
    ROW_LOOP_END
}

static unsigned row_blocks(long P, int G) {
    const long per_block = 4 * (64 / G);
    long blocks = (P + per_block - 1) / per_block;
    return (unsigned)(blocks > 16384 ? 16384 : blocks);
}

// the lane-group width of a row of nch 8-channel pieces
static int row_group(int nch) {
    int g = 1;
    while (g < nch && g < 64) g <<= 1;
    return g;
}

#define GATE_CASE(KERNEL, G, NK) hipLaunchKernelGGL((KERNEL<G, NK>), dim3(row_blocks(p.P, G)), dim3(256), 0, stream, p)
#define GATE_DISPATCH(KERNEL)                       \
    do {                                            \
        const int nch = p.C / 8;                    \
        if (nch > 128) GATE_CASE(KERNEL, 64, 4);    \
        else if (nch > 64) GATE_CASE(KERNEL, 64, 2);\
        else switch (row_group(nch)) {              \
            case 1: GATE_CASE(KERNEL, 1, 1); break; \
            case 2: GATE_CASE(KERNEL, 2, 1); break; \
            case 4: GATE_CASE(KERNEL, 4, 1); break; \
            case 8: GATE_CASE(KERNEL, 8, 1); break; \
            case 16: GATE_CASE(KERNEL, 16, 1); break;\
            case 32: GATE_CASE(KERNEL, 32, 1); break;\
            default: GATE_CASE(KERNEL, 64, 1); break;\
        }                                           \
    } while (0)

extern "C" int uenc_softmax_gate_fwd(const void* a, int a_dtype, const void* b, int b_dtype, const void* z, int z_dtype, void* res, void* g,
                                     int out_dtype, long P, int C, hipStream_t stream) {
    UENC_CHECK_ARG(a && b && z && res && g && P > 0 && C > 0 && C % 8 == 0 && C <= 2048);
    UENC_CHECK_ARG(dh_dtype(a_dtype) && dh_dtype(b_dtype) && dh_dtype(z_dtype) && dh_dtype(out_dtype));
    UENC_CHECK_ARG(dh_aligned(a) && dh_aligned(b) && dh_aligned(z) && dh_aligned(res) && dh_aligned(g));
    RowP p{a, a_dtype == UENC_F32, b, b_dtype == UENC_F32, z, z_dtype == UENC_F32, nullptr, 0, nullptr, res, g, out_dtype == UENC_F32, P, C};
    GATE_DISPATCH(softmax_gate_fwd_kernel);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_softmax_gate_bwd(const void* dg, int dg_dtype, const void* d_res_in, int d_res_in_dtype, const void* z, int z_dtype,
                                     const void* res, int res_dtype, void* d_res, void* d_z, int out_dtype, long P, int C, hipStream_t stream) {
    UENC_CHECK_ARG(dg && z && res && d_res && d_z && P > 0 && C > 0 && C % 8 == 0 && C <= 2048);
    UENC_CHECK_ARG(dh_dtype(dg_dtype) && (!d_res_in || dh_dtype(d_res_in_dtype)) && dh_dtype(z_dtype) && dh_dtype(res_dtype) && dh_dtype(out_dtype));
    UENC_CHECK_ARG(dh_aligned(dg) && dh_aligned(d_res_in) && dh_aligned(z) && dh_aligned(res) && dh_aligned(d_res) && dh_aligned(d_z));
    RowP p{dg, dg_dtype == UENC_F32, d_res_in, d_res_in_dtype == UENC_F32, z, z_dtype == UENC_F32, res, res_dtype == UENC_F32, nullptr,
           d_res, d_z, out_dtype == UENC_F32, P, C};
    GATE_DISPATCH(softmax_gate_bwd_kernel);
    UENC_LAUNCH_RET();
}

static void head_launch(const RowP& p, int backward, hipStream_t stream) {
    switch (row_group(p.C / 8)) {
        case 1: hipLaunchKernelGGL(soft_att_depth_kernel<1>, dim3(row_blocks(p.P, 1)), dim3(256), 0, stream, p, backward); break;
        case 2: hipLaunchKernelGGL(soft_att_depth_kernel<2>, dim3(row_blocks(p.P, 2)), dim3(256), 0, stream, p, backward); break;
        case 4: hipLaunchKernelGGL(soft_att_depth_kernel<4>, dim3(row_blocks(p.P, 4)), dim3(256), 0, stream, p, backward); break;
        default: hipLaunchKernelGGL(soft_att_depth_kernel<8>, dim3(row_blocks(p.P, 8)), dim3(256), 0, stream, p, backward); break;
    }
}

extern "C" int uenc_soft_att_depth_fwd(const void* z, int z_dtype, const float* grid, float* disp, long P, int D, hipStream_t stream) {
    UENC_CHECK_ARG(z && grid && disp && P > 0 && D > 0 && D % 8 == 0 && D <= 64);
    UENC_CHECK_ARG(dh_dtype(z_dtype) && dh_aligned(z) && dh_aligned(grid));
    RowP p{nullptr, 1, nullptr, 0, z, z_dtype == UENC_F32, nullptr, 0, grid, disp, nullptr, 1, P, D};
    head_launch(p, 0, stream);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_soft_att_depth_bwd(const float* ddisp, const void* z, int z_dtype, const float* grid, void* dz, int dz_dtype, long P, int D,
                                       hipStream_t stream) {
    UENC_CHECK_ARG(ddisp && z && grid && dz && P > 0 && D > 0 && D % 8 == 0 && D <= 64);
    UENC_CHECK_ARG(dh_dtype(z_dtype) && dh_dtype(dz_dtype) && dh_aligned(z) && dh_aligned(grid) && dh_aligned(dz));
    RowP p{ddisp, 1, nullptr, 0, z, z_dtype == UENC_F32, nullptr, 0, grid, dz, nullptr, dz_dtype == UENC_F32, P, D};
    head_launch(p, 1, stream);
    UENC_LAUNCH_RET();
}
