// Nearest-neighbour top-down merge of the plain FPN pixel decoders on channels-last token maps (gfx950), forward and adjoint.
//
// Reference: model/modeling/pixel_decoder/fpn.py:151 and :304, y = cur_fpn + F.interpolate(y, size=cur_fpn.shape[-2:], mode="nearest")
// (the MSDeformAttn decoder merges bilinearly: csrc/fpn.hip).  The source index of a destination index is exactly ATen's
// nearest_neighbor_compute_source_index: min(int(floorf(dst * ((float)Hs / H))), Hs - 1), the scale a float division, the product fp32.
// Both kernels are streaming passes: one thread = 4 consecutive channels of one pixel.
#include "common.h"

struct NrP {
    const void* a; int a_f32;            // (B, H, W, C) lateral map
    const void* prev; int prev_f32;      // (B, Hs, Ws, C) coarser map
    void* out; int out_f32;              // forward: (B, H, W, C); adjoint: unused
    const void* dy; int dy_f32;          // adjoint: (B, H, W, C)
    float* dprev;                        // adjoint: (B, Hs, Ws, C) fp32, written
    int B, H, W, Hs, Ws, C;
};

__device__ __forceinline__ float4 nr_ld4(const void* base, int is_f32, long idx) {
    if (is_f32) return *(const float4*)((const float*)base + idx);
    const bf16x4 v = *(const bf16x4*)((const bf16*)base + idx);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}

__device__ __forceinline__ int nearest_src(int dst, float scale, int n_in) { return min((int)floorf((float)dst * scale), n_in - 1); }

__global__ __launch_bounds__(256) void merge_nearest_fwd_kernel(NrP p) {
    const int cqn = p.C >> 2;
    const long total = (long)p.B * p.H * p.W * cqn;
    const float sy = (float)p.Hs / (float)p.H, sx = (float)p.Ws / (float)p.W;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int cq = (int)(t % cqn);
        long r = t / cqn;
        const int x = (int)(r % p.W); r /= p.W;
        const int y = (int)(r % p.H);
        const int b = (int)(r / p.H);
        const int ys = nearest_src(y, sy, p.Hs), xs = nearest_src(x, sx, p.Ws);
        const float4 u = nr_ld4(p.a, p.a_f32, t * 4);
        const float4 v = nr_ld4(p.prev, p.prev_f32, (((long)b * p.Hs + ys) * p.Ws + xs) * p.C + cq * 4);
        const float4 o = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
        if (p.out_f32) *(float4*)((float*)p.out + t * 4) = o;
        else {
            bf16x4 ob; ob[0] = (bf16)o.x; ob[1] = (bf16)o.y; ob[2] = (bf16)o.z; ob[3] = (bf16)o.w;
            *(bf16x4*)((bf16*)p.out + t * 4) = ob;
        }
    }
}

// candidate destinations of source index i: dst * scale in [i, i + 1), widened by one on either side for the fp32 rounding of the
// forward's product; the last source index also takes every destination the forward clamps to it
__device__ __forceinline__ void nearest_range(int i, int n_in, int n_out, float scale, int& lo, int& hi) {
    const float inv = 1.0f / scale;
    lo = (int)floorf((float)i * inv) - 1;
    hi = (int)ceilf((float)(i + 1) * inv) + 1;
    if (i == n_in - 1) hi = n_out - 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_out - 1 ? n_out - 1 : hi;
}

// Gather form (no atomics): every source pixel adds, in fp32 and in row-major order of the destination (oy ascending, then ox
// ascending), the dy of the destination pixels whose recomputed forward index is this pixel.
__global__ __launch_bounds__(256) void merge_nearest_bwd_kernel(NrP p) {
    const int cqn = p.C >> 2;
    const long total = (long)p.B * p.Hs * p.Ws * cqn;
    const float sy = (float)p.Hs / (float)p.H, sx = (float)p.Ws / (float)p.W;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int cq = (int)(t % cqn);
        long r = t / cqn;
        const int j = (int)(r % p.Ws); r /= p.Ws;
        const int i = (int)(r % p.Hs);
        const int b = (int)(r / p.Hs);
        int ylo, yhi, xlo, xhi;
        nearest_range(i, p.Hs, p.H, sy, ylo, yhi);
        nearest_range(j, p.Ws, p.W, sx, xlo, xhi);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int oy = ylo; oy <= yhi; ++oy) {
            if (nearest_src(oy, sy, p.Hs) != i) continue;
            for (int ox = xlo; ox <= xhi; ++ox) {
                if (nearest_src(ox, sx, p.Ws) != j) continue;
                const float4 d = nr_ld4(p.dy, p.dy_f32, (((long)b * p.H + oy) * p.W + ox) * p.C + cq * 4);
                acc.x += d.x; acc.y += d.y; acc.z += d.z; acc.w += d.w;
            }
        }
        *(float4*)(p.dprev + t * 4) = acc;
    }
}

static bool nr_dtype(int d) { return d == UENC_F32 || d == UENC_BF16; }

// out (B, H, W, C) = a (B, H, W, C) + nearest_resize(prev (B, Hs, Ws, C)) to (H, W); the sum is taken in fp32.
extern "C" int uenc_merge_nearest_tokens_fwd(const void* a, int a_dtype, const void* prev, int prev_dtype, void* out, int out_dtype, int B,
                                             int H, int W, int Hs, int Ws, int C, hipStream_t stream) {
    UENC_CHECK_ARG(a && prev && out && B > 0 && H > 0 && W > 0 && Hs > 0 && Ws > 0 && C > 0 && C % 4 == 0);
    UENC_CHECK_ARG(nr_dtype(a_dtype) && nr_dtype(prev_dtype) && nr_dtype(out_dtype));
    UENC_CHECK_ARG(((uintptr_t)a & (a_dtype == UENC_F32 ? 15 : 7)) == 0 && ((uintptr_t)prev & (prev_dtype == UENC_F32 ? 15 : 7)) == 0 &&
                   ((uintptr_t)out & (out_dtype == UENC_F32 ? 15 : 7)) == 0);
    NrP p{a, a_dtype == UENC_F32, prev, prev_dtype == UENC_F32, out, out_dtype == UENC_F32, nullptr, 0, nullptr, B, H, W, Hs, Ws, C};
    const long total = (long)B * H * W * (C / 4);
    long blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(merge_nearest_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    UENC_LAUNCH_RET();
}

// dprev (B, Hs, Ws, C) fp32 (every element written) = adjoint of nearest_resize (Hs, Ws) -> (H, W) applied to dy (B, H, W, C).
extern "C" int uenc_merge_nearest_tokens_bwd(const void* dy, int dy_dtype, float* dprev, int B, int H, int W, int Hs, int Ws, int C,
                                             hipStream_t stream) {
    UENC_CHECK_ARG(dy && dprev && B > 0 && H > 0 && W > 0 && Hs > 0 && Ws > 0 && C > 0 && C % 4 == 0);
    UENC_CHECK_ARG(nr_dtype(dy_dtype) && ((uintptr_t)dy & (dy_dtype == UENC_F32 ? 15 : 7)) == 0 && ((uintptr_t)dprev & 15) == 0);
    NrP p{nullptr, 0, nullptr, 0, nullptr, 0, dy, dy_dtype == UENC_F32, dprev, B, H, W, Hs, Ws, C};
    const long total = (long)B * Hs * Ws * (C / 4);
    long blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(merge_nearest_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    UENC_LAUNCH_RET();
}
