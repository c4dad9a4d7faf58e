// MonodepthLoss hot path (reference model/modeling/monodepth_loss.py:427-517, 671-680, 734-777), fp32, no float atomics anywhere.
//   uenc_view_synth_fwd / _bwd   per full-resolution pixel of every (scale, frame, image): bilinear disparity upsample (align_corners =
//                                False), disp_to_depth, back-projection, the three flow cases, projection(s), border-padded colour sampling
//                                (align_corners = True).  Backward: stage A per full-resolution pixel (+ per-block partial sums for
//                                cam_T_cam), stage B gathers every low-resolution map's gradient over its bounded footprint and adds the
//                                partials in a fixed order.
//   uenc_photo_loss_fwd / _bwd   0.85 mean_c SSIM + 0.15 mean_c L1 of every candidate over LDS tiles, the minimum with its index, and a
//                                block-partial mean per scale.  Backward through the selected candidate only, SSIM's 3x3 footprint
//                                gathered per source pixel (a reflected border pixel counts once per window position it fills).
#include "common.h"
#include <string.h>

#define MD_MAX_S 4
#define MD_MAX_F 2
#define MD_THREADS 256

struct VsDesc {                     // 67 pointers, filled by the caller on the host, passed by value
    const float* disp[MD_MAX_S];
    const float* cflow[MD_MAX_S * MD_MAX_F];
    const float* mask[MD_MAX_S * MD_MAX_F];
    const float* T;
    const float* K;
    const float* invK;
    const float* src;
    float* color;
    float* sample;
    float* sample_ego;
    float* sample_cmp;
    float* depth;
    float* residual[MD_MAX_S * MD_MAX_F];
    const float* gcolor;
    const float* gres[MD_MAX_S * MD_MAX_F];
    float* gdisp[MD_MAX_S];
    float* gcflow[MD_MAX_S * MD_MAX_F];
    float* gmask[MD_MAX_S * MD_MAX_F];
    float* gT;
};

// torch's upsample_bilinear2d source index for align_corners = False and an integer factor r (scale = 1 / r exactly)
__device__ __forceinline__ void up_index(int x, int r, int n, int& i0, int& i1, float& l) {
    float s = ((float)x + 0.5f) * (1.0f / (float)r) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i0 = i0 > n - 1 ? n - 1 : i0;
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    l = s - (float)i0;
}
__device__ __forceinline__ float bilerp(const float* __restrict__ p, int w, int y0, int y1, float ly, int x0, int x1, float lx) {
    return (1.f - ly) * ((1.f - lx) * p[y0 * w + x0] + lx * p[y0 * w + x1]) + ly * ((1.f - lx) * p[y1 * w + x0] + lx * p[y1 * w + x1]);
}

struct Proj {
    float sx, sy;                   // grid_sample coordinates in [-1, 1]
    float px, py, iz;               // camera-plane coordinates before the division by (W - 1, H - 1), and 1 / (z + eps)
};
__device__ __forceinline__ Proj project(const float* __restrict__ K, const float P[4], int H, int W) {
    const float cx = K[0] * P[0] + K[1] * P[1] + K[2] * P[2] + K[3] * P[3];
    const float cy = K[4] * P[0] + K[5] * P[1] + K[6] * P[2] + K[7] * P[3];
    const float cz = K[8] * P[0] + K[9] * P[1] + K[10] * P[2] + K[11] * P[3];
    Proj r;
    r.iz = 1.0f / (cz + 1e-7f);
    r.px = cx * r.iz;
    r.py = cy * r.iz;
    r.sx = (r.px / (float)(W - 1) - 0.5f) * 2.f;
    r.sy = (r.py / (float)(H - 1) - 0.5f) * 2.f;
    return r;
}
__device__ __forceinline__ void transform(const float* __restrict__ T, const float X[3], float P[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) P[i] = T[4 * i] * X[0] + T[4 * i + 1] * X[1] + T[4 * i + 2] * X[2] + T[4 * i + 3];
}
// grid_sample's unnormalise (align_corners = True) + border clip; `live` = 0 where the clip stops the gradient
__device__ __forceinline__ float unnorm_clip(float g, int n, float& live) {
    float v = ((g + 1.f) / 2.f) * (float)(n - 1);
    live = 1.f;
    if (!(v > 0.f)) { v = 0.f; live = 0.f; }
    else if (v >= (float)(n - 1)) { v = (float)(n - 1); live = 0.f; }
    return v;
}

// everything of one pixel the forward and the backward share
struct PixelGeom {
    float dv, depth, ray[3], X[3];
    int y0, y1, x0, x1;
    float ly, lx;
};
__device__ __forceinline__ PixelGeom pixel_geom(const float* __restrict__ disp, const float* __restrict__ iK, int x, int y, int r, int h, int w) {
    PixelGeom g;
    up_index(y, r, h, g.y0, g.y1, g.ly);
    up_index(x, r, w, g.x0, g.x1, g.lx);
    g.dv = bilerp(disp, w, g.y0, g.y1, g.ly, g.x0, g.x1, g.lx);
    g.depth = 1.0f / (0.01f + 9.99f * g.dv);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        g.ray[i] = iK[4 * i] * (float)x + iK[4 * i + 1] * (float)y + iK[4 * i + 2];
        g.X[i] = g.depth * g.ray[i];
    }
    return g;
}

template <int MODE>
__global__ __launch_bounds__(MD_THREADS) void view_synth_fwd_kernel(const VsDesc d, int S, int NF, int B, int H, int W) {
    const int item = blockIdx.y, s = item / (NF * B), f = (item / B) % NF, b = item % B;
    const int p = blockIdx.x * MD_THREADS + threadIdx.x;
    const int HW = H * W;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W, r = 1 << s, h = H >> s, w = W >> s, sf = s * NF + f;
    const float* K = d.K + 16 * b;
    const float* T = d.T + 16 * (f * B + b);
    const PixelGeom g = pixel_geom(d.disp[s] + (size_t)b * h * w, d.invK + 16 * b, x, y, r, h, w);
    if (f == 0) d.depth[((size_t)s * B + b) * HW + p] = g.depth;
    const size_t it = (size_t)item * HW + p;
    float P[4];
    Proj pr;
    if (MODE == 0) {
        transform(T, g.X, P);
        pr = project(K, P, H, W);
    } else {
        transform(T, g.X, P);
        const Proj pe = project(K, P, H, W);
        reinterpret_cast<float2*>(d.sample_ego)[it] = make_float2(pe.sx, pe.sy);
        float res[3], Xc[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float cf = bilerp(d.cflow[sf] + ((size_t)b * 3 + c) * h * w, w, g.y0, g.y1, g.ly, g.x0, g.x1, g.lx);
            res[c] = cf - (P[c] - g.X[c]);
            Xc[c] = g.X[c] + cf;
            d.residual[sf][((size_t)b * 3 + c) * HW + p] = res[c];
        }
        Xc[3] = 1.f;
        const Proj pc = project(K, Xc, H, W);
        reinterpret_cast<float2*>(d.sample_cmp)[it] = make_float2(pc.sx, pc.sy);
        if (MODE == 1) {
            pr = pc;
        } else {
            const float m = bilerp(d.mask[sf] + (size_t)b * h * w, w, g.y0, g.y1, g.ly, g.x0, g.x1, g.lx);
            float Xm[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) Xm[c] = g.X[c] + res[c] * m;
            transform(T, Xm, P);
            pr = project(K, P, H, W);
        }
    }
    reinterpret_cast<float2*>(d.sample)[it] = make_float2(pr.sx, pr.sy);
    float lvx, lvy;
    const float ix = unnorm_clip(pr.sx, W, lvx), iy = unnorm_clip(pr.sy, H, lvy);
    const int x0 = (int)floorf(ix), y0 = (int)floorf(iy);
    const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;      // a tap beyond the border has weight 0
    const float tx = ix - (float)x0, ty = iy - (float)y0;
    const float* src = d.src + (size_t)(f * B + b) * 3 * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* q = src + (size_t)c * HW;
        d.color[((size_t)item * 3 + c) * HW + p] =
            q[y0 * W + x0] * (1.f - tx) * (1.f - ty) + q[y0 * W + x1] * tx * (1.f - ty) + q[y1 * W + x0] * (1.f - tx) * ty + q[y1 * W + x1] * tx * ty;
    }
}

// gradient of the projection: d(loss)/d(P[0..3]) from d(loss)/d(pixel x, y)
__device__ __forceinline__ void project_bwd(const float* __restrict__ K, const Proj& pr, float gx, float gy, float dP[4]) {
    const float dcx = gx * pr.iz, dcy = gy * pr.iz, dcz = -(gx * pr.px + gy * pr.py) * pr.iz;
#pragma unroll
    for (int j = 0; j < 4; ++j) dP[j] = K[j] * dcx + K[4 + j] * dcy + K[8 + j] * dcz;
}

// Stage A.  ws planes (each S * NF * B * H * W): 0 d(disp upsampled), 1..3 d(complete flow upsampled), 4 d(mask upsampled); then the
// cam_T_cam partials (S * NF * B * nblk * 16).
template <int MODE>
__global__ __launch_bounds__(MD_THREADS) void view_synth_bwd_pixel_kernel(const VsDesc d, int S, int NF, int B, int H, int W, float* __restrict__ ws) {
    const int item = blockIdx.y, s = item / (NF * B), f = (item / B) % NF, b = item % B;
    const int p = blockIdx.x * MD_THREADS + threadIdx.x;
    const int HW = H * W;
    const size_t plane = (size_t)S * NF * B * HW;
    float gT[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) gT[i] = 0.f;
    if (p < HW) {
        const int y = p / W, x = p - y * W, r = 1 << s, h = H >> s, w = W >> s, sf = s * NF + f;
        const float* K = d.K + 16 * b;
        const float* T = d.T + 16 * (f * B + b);
        const PixelGeom g = pixel_geom(d.disp[s] + (size_t)b * h * w, d.invK + 16 * b, x, y, r, h, w);
        float P[4], Pe[4] = {0.f, 0.f, 0.f, 0.f}, cf[3] = {0.f, 0.f, 0.f}, res[3] = {0.f, 0.f, 0.f}, Xm[3], m = 0.f;
        Proj pr;
        if (MODE == 0) {
            transform(T, g.X, P);
            pr = project(K, P, H, W);
        } else {
            transform(T, g.X, Pe);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                cf[c] = bilerp(d.cflow[sf] + ((size_t)b * 3 + c) * h * w, w, g.y0, g.y1, g.ly, g.x0, g.x1, g.lx);
                res[c] = cf[c] - (Pe[c] - g.X[c]);
            }
            if (MODE == 1) {
#pragma unroll
                for (int c = 0; c < 3; ++c) P[c] = g.X[c] + cf[c];
                P[3] = 1.f;
            } else {
                m = bilerp(d.mask[sf] + (size_t)b * h * w, w, g.y0, g.y1, g.ly, g.x0, g.x1, g.lx);
#pragma unroll
                for (int c = 0; c < 3; ++c) Xm[c] = g.X[c] + res[c] * m;
                transform(T, Xm, P);
            }
            pr = project(K, P, H, W);
        }
        // colour sampling backward: d(loss)/d(ix, iy)
        float lvx, lvy;
        const float ix = unnorm_clip(pr.sx, W, lvx), iy = unnorm_clip(pr.sy, H, lvy);
        const int x0 = (int)floorf(ix), y0 = (int)floorf(iy);
        const bool inx = x0 + 1 < W, iny = y0 + 1 < H;
        const int x1 = inx ? x0 + 1 : W - 1, y1 = iny ? y0 + 1 : H - 1;
        const float tx = ix - (float)x0, ty = iy - (float)y0;
        const float* src = d.src + (size_t)(f * B + b) * 3 * HW;
        float gx = 0.f, gy = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* q = src + (size_t)c * HW;
            const float go = d.gcolor[((size_t)item * 3 + c) * HW + p];
            const float v00 = q[y0 * W + x0], v01 = inx ? q[y0 * W + x1] : 0.f, v10 = iny ? q[y1 * W + x0] : 0.f, v11 = (inx && iny) ? q[y1 * W + x1] : 0.f;
            gx += go * ((v01 - v00) * (1.f - ty) + (v11 - v10) * ty);
            gy += go * ((v10 - v00) * (1.f - tx) + (v11 - v01) * tx);
        }
        // normalise by (W - 1) and x 2, then grid_sample's (W - 1) / 2: the factors cancel
        gx *= lvx;
        gy *= lvy;
        float dP[4], dX[3] = {0.f, 0.f, 0.f}, dcf[3] = {0.f, 0.f, 0.f}, dm = 0.f;
        project_bwd(K, pr, gx, gy, dP);
        float gr[3] = {0.f, 0.f, 0.f};                   // d(loss)/d(residual flow) arriving from the regularisers
        if (MODE >= 1 && d.gres[sf] != nullptr) {
#pragma unroll
            for (int c = 0; c < 3; ++c) gr[c] = d.gres[sf][((size_t)b * 3 + c) * HW + p];
        }
        if (MODE == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                gT[4 * i] = dP[i] * g.X[0]; gT[4 * i + 1] = dP[i] * g.X[1]; gT[4 * i + 2] = dP[i] * g.X[2]; gT[4 * i + 3] = dP[i];
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) dX[j] = T[j] * dP[0] + T[4 + j] * dP[1] + T[8 + j] * dP[2] + T[12 + j] * dP[3];
        } else {
            float dres[3];
            if (MODE == 1) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { dX[c] = dP[c]; dcf[c] = dP[c]; dres[c] = gr[c]; }
            } else {
                float dXm[3];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    gT[4 * i] = dP[i] * Xm[0]; gT[4 * i + 1] = dP[i] * Xm[1]; gT[4 * i + 2] = dP[i] * Xm[2]; gT[4 * i + 3] = dP[i];
                }
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    dXm[j] = T[j] * dP[0] + T[4 + j] * dP[1] + T[8 + j] * dP[2] + T[12 + j] * dP[3];
                    dX[j] = dXm[j];
                    dm += dXm[j] * res[j];
                    dres[j] = dXm[j] * m + gr[j];
                }
            }
            // residual = cf - (T X - X): d(cf) += dres, d(ego) = -dres
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dcf[c] += dres[c];
                gT[4 * c] -= dres[c] * g.X[0]; gT[4 * c + 1] -= dres[c] * g.X[1]; gT[4 * c + 2] -= dres[c] * g.X[2]; gT[4 * c + 3] -= dres[c];
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) dX[j] += dres[j] - (T[j] * dres[0] + T[4 + j] * dres[1] + T[8 + j] * dres[2]);
        }
        const float ddepth = dX[0] * g.ray[0] + dX[1] * g.ray[1] + dX[2] * g.ray[2];
        const size_t it = (size_t)item * HW + p;
        ws[it] = -ddepth * g.depth * g.depth * 9.99f;
        if (MODE >= 1) {
            ws[plane + it] = dcf[0]; ws[2 * plane + it] = dcf[1]; ws[3 * plane + it] = dcf[2];
        }
        if (MODE == 2) ws[4 * plane + it] = dm;
    }
    // per-block partial sums of d(cam_T_cam): lanes, then the four waves in order
    __shared__ float red[MD_THREADS / 64][16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float v = wave_sum(gT[i]);
        if (lane == 0) red[wv][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        float v = red[0][threadIdx.x];
        for (int k = 1; k < MD_THREADS / 64; ++k) v += red[k][threadIdx.x];
        ws[5 * plane + ((size_t)item * gridDim.x + blockIdx.x) * 16 + threadIdx.x] = v;
    }
}

// weight of low-resolution index i in the upsampled value at full-resolution index x
__device__ __forceinline__ float up_weight(int x, int r, int n, int i) {
    int i0, i1;
    float l;
    up_index(x, r, n, i0, i1, l);
    return (i0 == i ? 1.f - l : 0.f) + (i1 == i ? l : 0.f);
}

// Stage B.  blockIdx.y < S * B: one low-resolution pixel per thread gathers its footprint (2r x 2r full-resolution pixels at most);
// blockIdx.y == S * B: d(cam_T_cam)[f][b][16] = partials added over scales and blocks in order.
template <int MODE>
__global__ __launch_bounds__(MD_THREADS) void view_synth_bwd_gather_kernel(const VsDesc d, int S, int NF, int B, int H, int W,
                                                                          const float* __restrict__ ws, int nblk) {
    const int HW = H * W;
    const size_t plane = (size_t)S * NF * B * HW;
    if ((int)blockIdx.y == S * B) {
        for (int t = blockIdx.x * MD_THREADS + threadIdx.x; t < NF * B * 16; t += gridDim.x * MD_THREADS) {
            const int e = t & 15, fb = t >> 4;
            float acc = 0.f;
            for (int s = 0; s < S; ++s) {
                const float* q = ws + 5 * plane + ((size_t)(s * NF * B + fb) * nblk) * 16 + e;
                for (int k = 0; k < nblk; ++k) acc += q[(size_t)k * 16];
            }
            d.gT[t] = acc;
        }
        return;
    }
    const int s = blockIdx.y / B, b = blockIdx.y % B, r = 1 << s, h = H >> s, w = W >> s;
    const int p = blockIdx.x * MD_THREADS + threadIdx.x;
    if (p >= h * w) return;
    const int i = p / w, j = p - i * w;
    const int ylo = max(0, r * i - r / 2), yhi = min(H - 1, r * i + r + r / 2 - 1);
    const int xlo = max(0, r * j - r / 2), xhi = min(W - 1, r * j + r + r / 2 - 1);
    float gd = 0.f;
    for (int f = 0; f < NF; ++f) {
        const size_t base = ((size_t)(s * NF + f) * B + b) * HW;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
        for (int y = ylo; y <= yhi; ++y) {
            const float wy = up_weight(y, r, h, i);
            if (wy == 0.f) continue;
            for (int x = xlo; x <= xhi; ++x) {
                const float wt = wy * up_weight(x, r, w, j);
                const size_t o = base + (size_t)y * W + x;
                a0 += wt * ws[o];
                if (MODE >= 1) { a1 += wt * ws[plane + o]; a2 += wt * ws[2 * plane + o]; a3 += wt * ws[3 * plane + o]; }
                if (MODE == 2) a4 += wt * ws[4 * plane + o];
            }
        }
        gd += a0;
        const int sf = s * NF + f;
        if (MODE >= 1) {
            float* o = d.gcflow[sf] + (size_t)b * 3 * h * w + p;
            o[0] = a1; o[(size_t)h * w] = a2; o[2 * (size_t)h * w] = a3;
        }
        if (MODE == 2) d.gmask[sf][(size_t)b * h * w + p] = a4;
    }
    d.gdisp[s][(size_t)b * h * w + p] = gd;
}

static bool vs_shape_ok(int S, int NF, int B, int H, int W, int mode) {
    if (S < 1 || S > MD_MAX_S || NF < 1 || NF > MD_MAX_F || B < 1 || B > 4096 || H < 2 || W < 2 || mode < 0 || mode > 2) return false;
    if (H % (1 << (S - 1)) != 0 || W % (1 << (S - 1)) != 0) return false;
    if ((long)H * W > (1L << 24) || (long)S * NF * B * 3 * H * W >= (1L << 31)) return false;
    return true;
}
static bool vs_inputs_ok(const VsDesc& d, int S, int NF, int mode) {
    if (!d.T || !d.K || !d.invK || !d.src) return false;
    for (int s = 0; s < S; ++s) {
        if (!d.disp[s]) return false;
        for (int f = 0; f < NF; ++f) {
            if (mode >= 1 && !d.cflow[s * NF + f]) return false;
            if (mode == 2 && !d.mask[s * NF + f]) return false;
        }
    }
    return true;
}

extern "C" long uenc_view_synth_workspace_floats(int S, int NF, int B, int H, int W) {
    if (!vs_shape_ok(S, NF, B, H, W, 0)) return -1;
    const long items = (long)S * NF * B, nblk = ceil_div64((long)H * W, MD_THREADS);
    return 5 * items * H * W + items * nblk * 16;
}

extern "C" int uenc_view_synth_fwd(const void* desc, int S, int NF, int B, int H, int W, int mode, hipStream_t stream) {
    UENC_CHECK_ARG(desc != nullptr && vs_shape_ok(S, NF, B, H, W, mode));
    VsDesc d;
    memcpy(&d, desc, sizeof(VsDesc));
    UENC_CHECK_ARG(vs_inputs_ok(d, S, NF, mode) && d.color && d.sample && d.depth);
    if (mode >= 1) {
        UENC_CHECK_ARG(d.sample_ego && d.sample_cmp);
        for (int i = 0; i < S * NF; ++i) UENC_CHECK_ARG(d.residual[i] != nullptr);
    }
    const dim3 grid((unsigned)ceil_div64((long)H * W, MD_THREADS), (unsigned)(S * NF * B));
    if (mode == 0) view_synth_fwd_kernel<0><<<grid, MD_THREADS, 0, stream>>>(d, S, NF, B, H, W);
    else if (mode == 1) view_synth_fwd_kernel<1><<<grid, MD_THREADS, 0, stream>>>(d, S, NF, B, H, W);
    else view_synth_fwd_kernel<2><<<grid, MD_THREADS, 0, stream>>>(d, S, NF, B, H, W);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_view_synth_bwd(const void* desc, int S, int NF, int B, int H, int W, int mode, float* workspace, long workspace_floats,
                                   hipStream_t stream) {
    UENC_CHECK_ARG(desc != nullptr && vs_shape_ok(S, NF, B, H, W, mode) && workspace != nullptr);
    UENC_CHECK_ARG(workspace_floats >= uenc_view_synth_workspace_floats(S, NF, B, H, W));
    VsDesc d;
    memcpy(&d, desc, sizeof(VsDesc));
    UENC_CHECK_ARG(vs_inputs_ok(d, S, NF, mode) && d.gcolor && d.gT);
    for (int s = 0; s < S; ++s) {
        UENC_CHECK_ARG(d.gdisp[s] != nullptr);
        for (int f = 0; f < NF; ++f) {
            if (mode >= 1) UENC_CHECK_ARG(d.gcflow[s * NF + f] != nullptr);
            if (mode == 2) UENC_CHECK_ARG(d.gmask[s * NF + f] != nullptr);
        }
    }
    const int nblk = (int)ceil_div64((long)H * W, MD_THREADS);
    const dim3 grid((unsigned)nblk, (unsigned)(S * NF * B)), grid2((unsigned)nblk, (unsigned)(S * B + 1));
    if (mode == 0) {
        view_synth_bwd_pixel_kernel<0><<<grid, MD_THREADS, 0, stream>>>(d, S, NF, B, H, W, workspace);
        view_synth_bwd_gather_kernel<0><<<grid2, MD_THREADS, 0, stream>>>(d, S, NF, B, H, W, workspace, nblk);
    } else if (mode == 1) {
        view_synth_bwd_pixel_kernel<1><<<grid, MD_THREADS, 0, stream>>>(d, S, NF, B, H, W, workspace);
        view_synth_bwd_gather_kernel<1><<<grid2, MD_THREADS, 0, stream>>>(d, S, NF, B, H, W, workspace, nblk);
    } else {
        view_synth_bwd_pixel_kernel<2><<<grid, MD_THREADS, 0, stream>>>(d, S, NF, B, H, W, workspace);
        view_synth_bwd_gather_kernel<2><<<grid2, MD_THREADS, 0, stream>>>(d, S, NF, B, H, W, workspace, nblk);
    }
    UENC_LAUNCH_RET();
}

// ---- photometric loss -----------------------------------------------------------------------------------------------------------------
#define PH_TX 32
#define PH_TY 8
#define PH_C1 1e-4f
#define PH_C2 9e-4f

__device__ __forceinline__ int reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);            // tiles that hang over the image: any valid address, the value is not used
}

struct SsimStats { float mx, my, vx, vy, cov; };
// 3x3 window statistics around (ly, lx) of two LDS planes with row stride LD (centred sums: no cancellation)
template <int LD>
__device__ __forceinline__ SsimStats window_stats(const float* __restrict__ px, const float* __restrict__ py, int ly, int lx) {
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) { sx += px[(ly + dy) * LD + lx + dx]; sy += py[(ly + dy) * LD + lx + dx]; }
    SsimStats st;
    st.mx = sx * (1.f / 9.f); st.my = sy * (1.f / 9.f);
    float vx = 0.f, vy = 0.f, cv = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const float a = px[(ly + dy) * LD + lx + dx] - st.mx, c = py[(ly + dy) * LD + lx + dx] - st.my;
            vx += a * a; vy += c * c; cv += a * c;
        }
    st.vx = vx * (1.f / 9.f); st.vy = vy * (1.f / 9.f); st.cov = cv * (1.f / 9.f);
    return st;
}

// candidate c of (scale s, image b): with auto-masking 0 .. NF - 1 are the source frames themselves, then the warped frames
__device__ __forceinline__ const float* candidate(const float* color, const float* src, int automask, int c, int s, int b, int NF, int B, size_t HW) {
    if (automask && c < NF) return src + ((size_t)c * B + b) * 3 * HW;
    const int f = automask ? c - NF : c;
    return color + (((size_t)s * NF + f) * B + b) * 3 * HW;
}

__global__ __launch_bounds__(MD_THREADS) void photo_loss_fwd_kernel(const float* __restrict__ color, const float* __restrict__ target,
                                                                    const float* __restrict__ src, const float* __restrict__ noise, int S, int NF,
                                                                    int B, int H, int W, int automask, unsigned char* __restrict__ argmin,
                                                                    float* __restrict__ partial) {
    constexpr int LD = PH_TX + 2, LR = PH_TY + 2;
    __shared__ float tg[3][LR * LD], pd[3][LR * LD];
    __shared__ float red[MD_THREADS / 64];
    const int tiles_x = (W + PH_TX - 1) / PH_TX;
    const int tx0 = (blockIdx.x % tiles_x) * PH_TX, ty0 = (blockIdx.x / tiles_x) * PH_TY;
    const int s = blockIdx.y / B, b = blockIdx.y % B;
    const size_t HW = (size_t)H * W;
    const int lx = threadIdx.x % PH_TX, ly = threadIdx.x / PH_TX, gx = tx0 + lx, gy = ty0 + ly;
    const bool valid = gx < W && gy < H;
    for (int i = threadIdx.x; i < 3 * LR * LD; i += MD_THREADS) {
        const int c = i / (LR * LD), rem = i - c * LR * LD, yy = rem / LD, xx = rem - yy * LD;
        tg[c][rem] = target[((size_t)b * 3 + c) * HW + (size_t)reflect(ty0 + yy - 1, H) * W + reflect(tx0 + xx - 1, W)];
    }
    const int NC = automask ? 2 * NF : NF;
    float best = 0.f;
    int arg = 0;
    for (int c = 0; c < NC; ++c) {
        const float* cand = candidate(color, src, automask, c, s, b, NF, B, HW);
        __syncthreads();
        for (int i = threadIdx.x; i < 3 * LR * LD; i += MD_THREADS) {
            const int ch = i / (LR * LD), rem = i - ch * LR * LD, yy = rem / LD, xx = rem - yy * LD;
            pd[ch][rem] = cand[(size_t)ch * HW + (size_t)reflect(ty0 + yy - 1, H) * W + reflect(tx0 + xx - 1, W)];
        }
        __syncthreads();
        float ssim = 0.f, l1 = 0.f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const SsimStats st = window_stats<LD>(pd[ch], tg[ch], ly + 1, lx + 1);
            const float n = (2.f * st.mx * st.my + PH_C1) * (2.f * st.cov + PH_C2);
            const float dn = (st.mx * st.mx + st.my * st.my + PH_C1) * (st.vx + st.vy + PH_C2);
            ssim += fminf(fmaxf((1.f - n / dn) * 0.5f, 0.f), 1.f);
            l1 += fabsf(tg[ch][(ly + 1) * LD + lx + 1] - pd[ch][(ly + 1) * LD + lx + 1]);
        }
        float v = 0.85f * (ssim * (1.f / 3.f)) + 0.15f * (l1 * (1.f / 3.f));
        if (automask && c < NF && valid) v += noise[(((size_t)s * B + b) * NF + c) * HW + (size_t)gy * W + gx] * 0.00001f;
        if (c == 0 || v < best) { best = v; arg = c; }
    }
    if (valid) argmin[((size_t)s * B + b) * HW + (size_t)gy * W + gx] = (unsigned char)arg;
    const float v = wave_sum(valid ? best : 0.f);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// p_photo[s] = (sum of the scale's B * tiles partials, fixed order) / (B * H * W)
__global__ __launch_bounds__(MD_THREADS) void photo_loss_mean_kernel(const float* __restrict__ partial, int n_per_scale, float inv_count,
                                                                     float* __restrict__ p_photo) {
    __shared__ float red[MD_THREADS];
    const float* q = partial + (size_t)blockIdx.x * n_per_scale;
    float acc = 0.f;
    for (int i = threadIdx.x; i < n_per_scale; i += MD_THREADS) acc += q[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = MD_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) p_photo[blockIdx.x] = red[0] * inv_count;
}

// how many window positions of centre p (p + {-1, 0, 1}, reflected) land on q
__device__ __forceinline__ int window_hits(int p, int q, int n) {
    return (reflect(p - 1, n) == q ? 1 : 0) + (p == q ? 1 : 0) + (reflect(p + 1, n) == q ? 1 : 0);
}

__global__ __launch_bounds__(MD_THREADS) void photo_loss_bwd_kernel(const float* __restrict__ color, const float* __restrict__ target,
                                                                    const unsigned char* __restrict__ argmin, const float* __restrict__ gp, int S,
                                                                    int NF, int B, int H, int W, int automask, float* __restrict__ gcolor) {
    constexpr int LD = PH_TX + 4, LR = PH_TY + 4;        // inputs: tile + 2
    constexpr int CD = PH_TX + 2, CR = PH_TY + 2;        // coefficients: tile + 1
    __shared__ float tg[3][LR * LD], pd[MD_MAX_F][3][LR * LD];
    __shared__ float cf[3][5][CR * CD];                  // per channel: a', b, c, mu_x, mu_y of the window centred there
    __shared__ int sel[CR * CD];                         // warped frame selected at that centre, -1 = none / identity / outside
    const int tiles_x = (W + PH_TX - 1) / PH_TX;
    const int tx0 = (blockIdx.x % tiles_x) * PH_TX, ty0 = (blockIdx.x / tiles_x) * PH_TY;
    const int s = blockIdx.y / B, b = blockIdx.y % B;
    const size_t HW = (size_t)H * W;
    for (int i = threadIdx.x; i < 3 * LR * LD; i += MD_THREADS) {
        const int c = i / (LR * LD), rem = i - c * LR * LD, yy = rem / LD, xx = rem - yy * LD;
        const size_t o = (size_t)c * HW + (size_t)reflect(ty0 + yy - 2, H) * W + reflect(tx0 + xx - 2, W);
        tg[c][rem] = target[(size_t)b * 3 * HW + o];
        for (int f = 0; f < NF; ++f) pd[f][c][rem] = color[(((size_t)s * NF + f) * B + b) * 3 * HW + o];
    }
    __syncthreads();
    const float g = gp[s] / ((float)B * (float)H * (float)W);
    for (int i = threadIdx.x; i < CR * CD; i += MD_THREADS) {
        const int yy = i / CD, xx = i - yy * CD, py = ty0 + yy - 1, px = tx0 + xx - 1;
        int f = -1;
        if (py >= 0 && py < H && px >= 0 && px < W) {
            const int a = argmin[((size_t)s * B + b) * HW + (size_t)py * W + px];
            f = automask ? a - NF : a;
            if (f >= NF) f = -1;
        }
        sel[i] = f;
        if (f < 0) continue;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const SsimStats st = window_stats<LD>(pd[f][ch], tg[ch], yy + 1, xx + 1);
            const float n1 = 2.f * st.mx * st.my + PH_C1, n2 = 2.f * st.cov + PH_C2;
            const float d1 = st.mx * st.mx + st.my * st.my + PH_C1, d2 = st.vx + st.vy + PH_C2;
            const float id = 1.f / (d1 * d2), Sv = n1 * n2 * id;
            const float l = (1.f - Sv) * 0.5f;
            const float G = (l >= 0.f && l <= 1.f) ? g * (0.85f / 3.f) * (-0.5f) : 0.f;       // d(loss)/d(SSIM) of this window
            cf[ch][0][i] = G * (2.f * st.my * n2 * id - 2.f * st.mx * Sv / d1);
            cf[ch][1][i] = G * (-Sv / d2);
            cf[ch][2][i] = G * (2.f * n1 * id);
            cf[ch][3][i] = st.mx;
            cf[ch][4][i] = st.my;
        }
    }
    __syncthreads();
    const int lx = threadIdx.x % PH_TX, ly = threadIdx.x / PH_TX, qx = tx0 + lx, qy = ty0 + ly;
    if (qx >= W || qy >= H) return;
    for (int f = 0; f < NF; ++f) {
        float acc[3] = {0.f, 0.f, 0.f};
        for (int dy = -1; dy <= 1; ++dy) {
            const int py = qy + dy;
            if (py < 0 || py >= H) continue;
            const int my = window_hits(py, qy, H);
            for (int dx = -1; dx <= 1; ++dx) {
                const int px = qx + dx;
                if (px < 0 || px >= W) continue;
                const int ci = (ly + 1 + dy) * CD + lx + 1 + dx;
                if (sel[ci] != f) continue;
                const float m = (float)(my * window_hits(px, qx, W)) * (1.f / 9.f);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float xq = pd[f][ch][(ly + 2) * LD + lx + 2], yq = tg[ch][(ly + 2) * LD + lx + 2];
                    acc[ch] += m * (cf[ch][0][ci] + 2.f * cf[ch][1][ci] * (xq - cf[ch][3][ci]) + cf[ch][2][ci] * (yq - cf[ch][4][ci]));
                }
            }
        }
        const bool mine = sel[(ly + 1) * CD + lx + 1] == f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float df = pd[f][ch][(ly + 2) * LD + lx + 2] - tg[ch][(ly + 2) * LD + lx + 2];
            const float sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
            gcolor[((((size_t)s * NF + f) * B + b) * 3 + ch) * HW + (size_t)qy * W + qx] = acc[ch] + (mine ? g * (0.15f / 3.f) * sg : 0.f);
        }
    }
}

static bool ph_shape_ok(int S, int NF, int B, int H, int W) {
    return S >= 1 && S <= MD_MAX_S && NF >= 1 && NF <= MD_MAX_F && B >= 1 && B <= 4096 && H >= 2 && W >= 2 && (long)H * W <= (1L << 24) &&
           (long)S * NF * B * 3 * H * W < (1L << 31) && (long)S * B <= 65535;
}
static long ph_tiles(int H, int W) { return ceil_div64(W, PH_TX) * ceil_div64(H, PH_TY); }

extern "C" long uenc_photo_loss_workspace_floats(int S, int B, int H, int W) {
    if (!ph_shape_ok(S, 1, B, H, W)) return -1;
    return (long)S * B * ph_tiles(H, W);
}

extern "C" int uenc_photo_loss_fwd(const float* color, const float* target, const float* src, const float* noise, int S, int NF, int B, int H,
                                   int W, int automask, float* workspace, long workspace_floats, unsigned char* argmin, float* p_photo,
                                   hipStream_t stream) {
    UENC_CHECK_ARG(ph_shape_ok(S, NF, B, H, W) && color && target && workspace && argmin && p_photo);
    UENC_CHECK_ARG(automask == 0 || (automask == 1 && src && noise));
    UENC_CHECK_ARG(workspace_floats >= uenc_photo_loss_workspace_floats(S, B, H, W));
    const long tiles = ph_tiles(H, W);
    photo_loss_fwd_kernel<<<dim3((unsigned)tiles, (unsigned)(S * B)), MD_THREADS, 0, stream>>>(color, target, src, noise, S, NF, B, H, W, automask,
                                                                                              argmin, workspace);
    photo_loss_mean_kernel<<<S, MD_THREADS, 0, stream>>>(workspace, (int)(B * tiles), 1.0f / ((float)B * (float)H * (float)W), p_photo);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_photo_loss_bwd(const float* color, const float* target, const unsigned char* argmin, const float* grad_p_photo, int S, int NF,
                                   int B, int H, int W, int automask, float* grad_color, hipStream_t stream) {
    UENC_CHECK_ARG(ph_shape_ok(S, NF, B, H, W) && color && target && argmin && grad_p_photo && grad_color && (automask == 0 || automask == 1));
    photo_loss_bwd_kernel<<<dim3((unsigned)ph_tiles(H, W), (unsigned)(S * B)), MD_THREADS, 0, stream>>>(color, target, argmin, grad_p_photo, S, NF, B,
                                                                                                       H, W, automask, grad_color);
    UENC_LAUNCH_RET();
}
