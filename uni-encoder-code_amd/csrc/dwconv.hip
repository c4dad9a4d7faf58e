// ConvNeXt block front end (reference model/modeling/backbone/convnext.py:41-45): 7x7 depthwise convolution, padding 3, on the fp32
// channels-last residual stream, fused with the LayerNorm over channels that follows it; its two backward kernels; and the layer-scale
// gradient step of the block's second pointwise layer.  No contraction dimension: VALU + LDS + bandwidth kernels, fp32 throughout.
//
// Tiling (all three convolution kernels): a workgroup of 256 threads owns an 8 x 8 pixel tile and walks the channels in slabs of 32.
// Per slab the (8+6) x (8+6) x 32 fp32 input halo (25 088 B) is staged in LDS once, so every input element is read from HBM / L2 once
// per tile instead of 49 times.  Thread t = (row r = t / 32, channel lane cl = t % 32) produces the 8 pixels of tile row r for channel
// c0 + cl: it slides along the row, reading 7 x 14 halo values from LDS for 8 x 49 multiply-adds.  The 32 lanes of a half-wave read 32
// consecutive floats of one halo pixel: ds_read_b32 banks are (address / 4) % 32 per 32-lane half, so the reads are conflict-free.
// A half-wave therefore holds whole channel rows of its 8 pixels (over the slab loop), and the LayerNorm statistics are half-wave
// butterfly sums: no cross-wave traffic.
#include "common.h"

namespace {

constexpr int TH = 8, TW = 8, CS = 32, HH = TH + 6, HW = TW + 6, NTHREADS = 256;
constexpr int HALO_FLOATS = HH * HW * CS;                 // 6272 floats = 25 088 B
constexpr int YLDS_MAX_C = 384;                           // y tile (64 pixels x C fp32) kept in LDS up to this width: 96 KB + the halo
constexpr int NACC = 50;                                  // 49 filter taps + the bias

struct DwP {
    const float* x;        // (B, H, W, C) input of the convolution
    const float* w;        // (C, 49)
    const float* b;        // (C) or NULL
    const float* gamma;    // LayerNorm weight / bias (forward only)
    const float* beta;
    const float* addend;   // transposed mode: optional (B, H, W, C) added to the result
    float* y;              // (B, H, W, C) convolution result
    void* h;               // forward: LN(y) as fp32 | bf16
    float2* stats;         // forward: (B*H*W) (mean, rstd)
    int h_f32;
    int B, H, W, C, tilesX, tilesY;
    float eps;
    int ylds;              // forward: the y tile stays in LDS between the sweeps
};

// stage the halo of tile (b, y0, x0), channels [c0, c0 + 32), zero outside the map and past C (C % 4 == 0: a float4 is in or out)
__device__ __forceinline__ void load_halo(float* xs, const float* __restrict__ x, int b, int y0, int x0, int c0, int H, int W, int C) {
    for (int i = threadIdx.x; i < HH * HW * (CS / 4); i += NTHREADS) {
        const int pix = i >> 3, q = i & 7;
        const int hy = pix / HW, hx = pix - hy * HW;
        const int gy = y0 + hy - 3, gx = x0 + hx - 3, c = c0 + q * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gy >= 0 && gy < H && gx >= 0 && gx < W && c < C)
            v = *reinterpret_cast<const float4*>(x + (((long)b * H + gy) * W + gx) * C + c);
        *reinterpret_cast<float4*>(xs + pix * CS + q * 4) = v;
    }
}

__device__ __forceinline__ float half_wave_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// FWD: y = conv(x) + b, h = LN_C(y), stats.  !FWD: y = conv with the flipped filter (the adjoint) + addend.
template <bool FWD>
__global__ __launch_bounds__(NTHREADS) void dwconv7_kernel(DwP p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;                       // halo
    float* ys = smem + HALO_FLOATS;         // FWD && ylds: [64 pixels][C]
    const int H = p.H, W = p.W, C = p.C;
    const int b = blockIdx.y;
    const int ty = blockIdx.x / p.tilesX, tx = blockIdx.x - ty * p.tilesX;
    const int y0 = ty * TH, x0 = tx * TW;
    const int cl = threadIdx.x & 31, r = threadIdx.x >> 5;
    const int gy = y0 + r;
    const long rowbase = (((long)b * H + gy) * W + x0) * C;       // element index of pixel (gy, x0), channel 0
    const int nslab = (C + CS - 1) / CS;
    float s[TW];
#pragma unroll
    for (int px = 0; px < TW; ++px) s[px] = 0.f;

    for (int sl = 0; sl < nslab; ++sl) {
        const int c0 = sl * CS, c = c0 + cl;
        const bool active = c < C;
        __syncthreads();
        load_halo(xs, p.x, b, y0, x0, c0, H, W, C);
        __syncthreads();
        float wr[49];
#pragma unroll
        for (int k = 0; k < 49; ++k) wr[k] = active ? p.w[(long)c * 49 + (FWD ? k : 48 - k)] : 0.f;
        float acc[TW];
        const float bias = (FWD && active && p.b) ? p.b[c] : 0.f;
#pragma unroll
        for (int px = 0; px < TW; ++px) acc[px] = bias;
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            float row[HW];
#pragma unroll
            for (int j = 0; j < HW; ++j) row[j] = xs[((r + ky) * HW + j) * CS + cl];
#pragma unroll
            for (int kx = 0; kx < 7; ++kx)
#pragma unroll
                for (int px = 0; px < TW; ++px) acc[px] = fmaf(row[px + kx], wr[ky * 7 + kx], acc[px]);
        }
#pragma unroll
        for (int px = 0; px < TW; ++px) {
            const bool valid = active && gy < H && x0 + px < W;
            const long idx = rowbase + (long)px * C + c;
            if (FWD) {
                if (valid) {
                    p.y[idx] = acc[px];
                    s[px] += acc[px];
                    if (p.ylds) ys[(r * TW + px) * C + c] = acc[px];
                }
            } else if (valid) {
                p.y[idx] = acc[px] + (p.addend ? p.addend[idx] : 0.f);
            }
        }
    }
    if (!FWD) return;

    // LayerNorm over the channel row of each pixel: this half-wave produced all of it.  The second and third sweep re-read the
    // thread's own y values, from LDS when the tile fits, else from the lines it has just written (L2).
    const float invC = 1.0f / (float)C;
    float mean[TW], q[TW];
#pragma unroll
    for (int px = 0; px < TW; ++px) { mean[px] = half_wave_sum(s[px]) * invC; q[px] = 0.f; }
    for (int sl = 0; sl < nslab; ++sl) {
        const int c = sl * CS + cl;
        if (c < C) {
#pragma unroll
            for (int px = 0; px < TW; ++px) {
                if (gy < H && x0 + px < W) {
                    const float v = p.ylds ? ys[(r * TW + px) * C + c] : p.y[rowbase + (long)px * C + c];
                    const float d = v - mean[px];
                    q[px] = fmaf(d, d, q[px]);
                }
            }
        }
    }
    float rstd[TW];
#pragma unroll
    for (int px = 0; px < TW; ++px) rstd[px] = rsqrtf(half_wave_sum(q[px]) * invC + p.eps);
    for (int sl = 0; sl < nslab; ++sl) {
        const int c = sl * CS + cl;
        if (c < C) {
            const float g = p.gamma[c], be = p.beta[c];
#pragma unroll
            for (int px = 0; px < TW; ++px) {
                if (gy < H && x0 + px < W) {
                    const long idx = rowbase + (long)px * C + c;
                    const float v = p.ylds ? ys[(r * TW + px) * C + c] : p.y[idx];
                    const float o = (v - mean[px]) * rstd[px] * g + be;
                    if (p.h_f32) reinterpret_cast<float*>(p.h)[idx] = o;
                    else reinterpret_cast<bf16*>(p.h)[idx] = (bf16)o;
                }
            }
        }
    }
    if (cl == 0 && gy < H) {
#pragma unroll
        for (int px = 0; px < TW; ++px)
            if (x0 + px < W) p.stats[((long)b * H + gy) * W + x0 + px] = make_float2(mean[px], rstd[px]);
    }
}

// Weight gradient, stage 1: workgroup (slab, nb) walks the tiles nb, nb + NB, ... and keeps the 49 tap sums and the bias sum of its 32
// channels in registers; one cross-wave reduction at the end, stored (no atomics) to ws[nb][50][C].
__global__ __launch_bounds__(NTHREADS) void dwconv7_wgrad_partial_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                         float* __restrict__ ws, int B, int H, int W, int C,
                                                                         int tilesX, int tilesY, int NB) {
    __shared__ __attribute__((aligned(16))) float xs[HALO_FLOATS];
    __shared__ float red[4][NACC][CS];
    const int c0 = blockIdx.x * CS, nb = blockIdx.y;
    const int cl = threadIdx.x & 31, r = threadIdx.x >> 5;
    const int c = c0 + cl;
    const bool active = c < C;
    const int ntiles = B * tilesX * tilesY;
    float acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.f;
    for (int tile = nb; tile < ntiles; tile += NB) {
        const int b = tile / (tilesX * tilesY), rem = tile - b * (tilesX * tilesY);
        const int ty = rem / tilesX, tx = rem - ty * tilesX;
        const int y0 = ty * TH, x0 = tx * TW, gy = y0 + r;
        __syncthreads();
        load_halo(xs, x, b, y0, x0, c0, H, W, C);
        __syncthreads();
        float g[TW];
        float gs = 0.f;
#pragma unroll
        for (int px = 0; px < TW; ++px) {
            const bool valid = active && gy < H && x0 + px < W;
            g[px] = valid ? dy[(((long)b * H + gy) * W + x0 + px) * C + c] : 0.f;
            gs += g[px];
        }
        acc[49] += gs;
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            float row[HW];
#pragma unroll
            for (int j = 0; j < HW; ++j) row[j] = xs[((r + ky) * HW + j) * CS + cl];
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                float a = 0.f;
#pragma unroll
                for (int px = 0; px < TW; ++px) a = fmaf(g[px], row[px + kx], a);
                acc[ky * 7 + kx] += a;
            }
        }
    }
    // rows r and r + 1 of a wave, then the 4 waves (fixed order)
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const float v = acc[k] + __shfl_xor(acc[k], 32);
        if ((threadIdx.x & 32) == 0) red[wv][k][cl] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NACC * CS; i += NTHREADS) {
        const int k = i >> 5, l = i & 31;
        if (c0 + l < C) ws[((long)nb * NACC + k) * C + c0 + l] = (red[0][k][l] + red[1][k][l]) + (red[2][k][l] + red[3][k][l]);
    }
}

// stage 2: dw[c][k] += sum_nb ws[nb][k][c] (k < 49), db[c] += sum_nb ws[nb][49][c], partials added in ascending nb
__global__ __launch_bounds__(256) void dwconv7_wgrad_final_kernel(const float* __restrict__ ws, float* __restrict__ dw, float* __restrict__ db,
                                                                  int C, int NB) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NACC * C) return;
    const int k = i / C, c = i - k * C;
    float sum = 0.f;
    for (int nb = 0; nb < NB; ++nb) sum += ws[((long)nb * NACC + k) * C + c];
    if (k < 49) dw[(long)c * 49 + k] += sum;
    else if (db) db[c] += sum;
}

// Layer scale folded into fc2 (W2' = gamma (.) W2 row-wise, b2' = gamma (.) b2): from dW2' (N, K) and db2' (N) of the folded layer,
//   gW2 += gamma (.) dW2',  gb2 += gamma (.) db2',  ggamma[n] += sum_k dW2'[n][k] W2[n][k] + db2'[n] b2[n].   One workgroup per row n.
__global__ __launch_bounds__(256) void layer_scale_grads_kernel(const float* __restrict__ dw2p, const float* __restrict__ db2p,
                                                                const float* __restrict__ w2, const float* __restrict__ b2,
                                                                const float* __restrict__ gamma, float* __restrict__ gw2,
                                                                float* __restrict__ gb2, float* __restrict__ ggamma, int K) {
    __shared__ float red[4];
    const int n = blockIdx.x;
    const float ga = gamma[n];
    float a = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) {
        const long i = (long)n * K + k;
        const float d = dw2p[i];
        if (gw2) gw2[i] += ga * d;
        a = fmaf(d, w2[i], a);
    }
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float d = db2p ? db2p[n] : 0.f;
        if (ggamma) ggamma[n] += (red[0] + red[1]) + (red[2] + red[3]) + d * (b2 ? b2[n] : 0.f);
        if (gb2) gb2[n] += ga * d;
    }
}

int conv_launch(bool fwd, DwP& p, hipStream_t stream) {
    p.tilesX = (p.W + TW - 1) / TW;
    p.tilesY = (p.H + TH - 1) / TH;
    p.ylds = fwd && p.C <= YLDS_MAX_C;
    const size_t shm = (size_t)(HALO_FLOATS + (p.ylds ? TH * TW * p.C : 0)) * sizeof(float);
    if (fwd) {
        static bool attr_set = false;
        if (!attr_set) {
            hipError_t e = hipFuncSetAttribute((const void*)dwconv7_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)((HALO_FLOATS + TH * TW * YLDS_MAX_C) * sizeof(float)));
            if (e != hipSuccess) return (int)e;
            attr_set = true;
        }
        hipLaunchKernelGGL(dwconv7_kernel<true>, dim3(p.tilesX * p.tilesY, p.B), dim3(NTHREADS), shm, stream, p);
    } else {
        hipLaunchKernelGGL(dwconv7_kernel<false>, dim3(p.tilesX * p.tilesY, p.B), dim3(NTHREADS), shm, stream, p);
    }
    UENC_LAUNCH_RET();
}

bool dw_shape_ok(int B, int H, int W, int C) {
    return B > 0 && B <= 65535 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && C <= 6144 && (long)((H + TH - 1) / TH) * ((W + TW - 1) / TW) < (1L << 31)
           && (long)B * H * W < (1L << 31);
}

int wgrad_blocks(int B, int H, int W) {
    const long nt = (long)B * ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
    return (int)(nt < 256 ? nt : 256);
}

}  // namespace

extern "C" int uenc_dwconv7_ln_fwd(const float* x, const float* w, const float* b, const float* gamma, const float* beta, float* y, void* h,
                                   int h_dtype, float* stats, int B, int H, int W, int C, float eps, hipStream_t stream) {
    UENC_CHECK_ARG(x && w && gamma && beta && y && h && stats && dw_shape_ok(B, H, W, C));
    UENC_CHECK_ARG(h_dtype == UENC_F32 || h_dtype == UENC_BF16);
    UENC_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)stats) & 15) == 0 && ((uintptr_t)h & 3) == 0);
    DwP p;
    p.x = x; p.w = w; p.b = b; p.gamma = gamma; p.beta = beta; p.addend = nullptr; p.y = y; p.h = h; p.stats = (float2*)stats;
    p.h_f32 = (h_dtype == UENC_F32); p.B = B; p.H = H; p.W = W; p.C = C; p.eps = eps;
    return conv_launch(true, p, stream);
}

extern "C" int uenc_dwconv7_ln_bwd_data(const void* dh, int dh_dtype, const float* y, const float* stats, const float* gamma, const float* w,
                                        const float* dout, float* dy, float* dx, float* dgamma, float* dbeta, float* part_ws,
                                        int defer_param_sums, int B, int H, int W, int C, hipStream_t stream) {
    UENC_CHECK_ARG(dh && y && stats && gamma && w && dy && dx && dw_shape_ok(B, H, W, C));
    UENC_CHECK_ARG(dh_dtype == UENC_F32 || dh_dtype == UENC_BF16);
    UENC_CHECK_ARG((dgamma == nullptr) == (dbeta == nullptr) && dy != dx);
    UENC_CHECK_ARG((((uintptr_t)dh | (uintptr_t)y | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)dout) & 15) == 0);
    // LayerNorm backward per pixel: dy (fp32, every element written), dgamma / dbeta with the conventions of uenc_layernorm_bwd
    const int rc = uenc_layernorm_bwd(dh, dh_dtype, y, UENC_F32, stats, gamma, nullptr, dy, UENC_F32, dgamma, dbeta, (long)B * H * W, C, nullptr,
                                      part_ws, defer_param_sums, stream);
    if (rc != UENC_OK) return rc;
    DwP p;
    p.x = dy; p.w = w; p.b = nullptr; p.gamma = p.beta = nullptr; p.addend = dout; p.y = dx; p.h = nullptr; p.stats = nullptr;
    p.h_f32 = 1; p.B = B; p.H = H; p.W = W; p.C = C; p.eps = 0.f;
    return conv_launch(false, p, stream);
}

extern "C" long uenc_dwconv7_bwd_weight_workspace_bytes(int B, int H, int W, int C) {
    if (!dw_shape_ok(B, H, W, C)) return 0;
    return (long)wgrad_blocks(B, H, W) * NACC * C * (long)sizeof(float);
}

extern "C" int uenc_dwconv7_bwd_weight(const float* dy, const float* x, float* dw, float* db, void* workspace, long workspace_bytes, int B, int H,
                                       int W, int C, hipStream_t stream) {
    UENC_CHECK_ARG(dy && x && dw && workspace && dw_shape_ok(B, H, W, C));
    UENC_CHECK_ARG(workspace_bytes >= uenc_dwconv7_bwd_weight_workspace_bytes(B, H, W, C));
    UENC_CHECK_ARG((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)workspace) & 15) == 0);
    const int NB = wgrad_blocks(B, H, W);
    const int tilesX = (W + TW - 1) / TW, tilesY = (H + TH - 1) / TH;
    hipLaunchKernelGGL(dwconv7_wgrad_partial_kernel, dim3((C + CS - 1) / CS, NB), dim3(NTHREADS), 0, stream, dy, x, (float*)workspace, B, H, W,
                       C, tilesX, tilesY, NB);
    hipLaunchKernelGGL(dwconv7_wgrad_final_kernel, dim3((NACC * C + 255) / 256), dim3(256), 0, stream, (const float*)workspace, dw, db, C, NB);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_layer_scale_grads(const float* dw2p, const float* db2p, const float* w2, const float* b2, const float* gamma, float* gw2,
                                      float* gb2, float* ggamma, int N, int K, hipStream_t stream) {
    UENC_CHECK_ARG(dw2p && w2 && gamma && N > 0 && K > 0 && (gw2 || gb2 || ggamma));
    UENC_CHECK_ARG(gw2 != dw2p && (db2p || !gb2));
    hipLaunchKernelGGL(layer_scale_grads_kernel, dim3(N), dim3(256), 0, stream, dw2p, db2p, w2, b2, gamma, gw2, gb2, ggamma, K);
    UENC_LAUNCH_RET();
}
