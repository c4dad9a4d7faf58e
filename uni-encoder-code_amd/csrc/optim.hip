// Fused AdamW with full-model gradient clipping (uenc.optim.FusedAdamW): the optimizer step of a training loop as three stream-ordered
// entry points whose every input lives on the device, so that a captured training step can end with its own weight update.
//
// What torch does from the host per tensor (torch.nan_to_num on every gradient, clip_grad_norm_ over all of them, torch.optim.AdamW)
// becomes
//   uenc_optim_advance      step += 1 and the bias corrections of that step (one workgroup),
//   uenc_optim_grad_sqnorm  sum of squares of the sanitised gradients -> total norm and clip coefficient (two stages, no atomics),
//   uenc_optim_adamw_step   one pass over parameter, gradient and both moments of every tensor.
// A device table of segments (one per parameter tensor) says where things are; a tile of OPT_TILE elements is mapped to its segment
// by binary search over the exclusive prefix sum of tile counts, as uenc_cast_multi does.  The gradient buffers are only read.
//
// Alignment.  A segment's tiles are laid over the index space j = i + a, a = the element offset of the parameter pointer from its
// 16-byte boundary, so every group of four j starts on a 16-byte boundary of the PARAMETER.  A group that lies wholly inside
// [0, n) moves as four-float vectors (the first and last group of a segment that starts or ends off such a boundary go element by
// element).  Gradient and moments may sit at any other 4-byte offset (views into a flat all-reduce bucket do): their vectors are
// declared 4-byte aligned, which global memory accepts for a 16-byte access.
#include "common.h"

#define OPT_TILE 4096            // elements per tile: 256 lanes x 4 groups of 4
#define OPT_MAX_GRID 2048

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
// Pointers read from the table are generic to the compiler; every one of them is HBM, so say so (global_* instead of flat_* accesses).
#define OPT_GLOBAL __attribute__((address_space(1)))
__device__ __forceinline__ f32x4u ld4(const float* p) { return *(const OPT_GLOBAL f32x4u*)p; }
__device__ __forceinline__ float ld1(const float* p) { return *(const OPT_GLOBAL float*)p; }
__device__ __forceinline__ void st4(float* p, f32x4u v) { *(OPT_GLOBAL f32x4u*)p = v; }
__device__ __forceinline__ void st1(float* p, float v) { *(OPT_GLOBAL float*)p = v; }

struct OptimSeg {
    float* p; const float* g; float* m; float* v;
    long n;                      // elements
    long tile_begin;             // exclusive prefix sum of ceil((n + a) / OPT_TILE)
    int group, pad;
};
static_assert(sizeof(OptimSeg) == 56, "descriptor layout is part of the ABI");

struct OptimState {
    long long step;              // optimizer steps taken (advanced by uenc_optim_advance)
    double norm;                 // total gradient norm of the last uenc_optim_grad_sqnorm (for logging)
    float clip_coef;             // min(1, max_norm / (norm + 1e-6)); stays 1 when clipping is off
    float inv_bc1;               // 1 / (1 - beta1^step)
    float inv_sqrt_bc2;          // 1 / sqrt(1 - beta2^step)
    float pad;
};
static_assert(sizeof(OptimState) == 32, "state block layout is part of the ABI");

__device__ __forceinline__ int find_segment(const OptimSeg* __restrict__ table, int n, long tix) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].tile_begin <= tix) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// torch.nan_to_num(g, nan=0, posinf=1e5, neginf=-1e5)
__device__ __forceinline__ float sanitise(float g) {
    if (g != g) return 0.f;
    if (g == __builtin_inff()) return 1e5f;
    if (g == -__builtin_inff()) return -1e5f;
    return g;
}

__device__ __forceinline__ int misalign4(const void* p) { return (int)(((uintptr_t)p >> 2) & 3); }

// ---- norm ------------------------------------------------------------------------------------------------------------------------
// Stage 1: workgroup b adds the squares of tiles b, b + grid, ... -- each lane in double, then a fixed-order tree over the workgroup --
// and writes partials[b].  The grid is a function of total_tiles alone, so the same input gives the same bits.
__global__ __launch_bounds__(256) void optim_sqnorm_partial_kernel(const OptimSeg* __restrict__ table, int n, long total_tiles,
                                                                  double* __restrict__ partials) {
    __shared__ double red[256];
    double acc = 0.0;
    for (long tix = blockIdx.x; tix < total_tiles; tix += gridDim.x) {
        const int s = find_segment(table, n, tix);
        const OptimSeg d = table[s];
        const int a = misalign4(d.p);
        const long j0 = (tix - d.tile_begin) * OPT_TILE;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long i = j0 + k * 1024 + threadIdx.x * 4 - a;
            if (i >= 0 && i + 4 <= d.n) {
                const f32x4u g = ld4(d.g + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) { const double x = (double)sanitise(g[e]); acc += x * x; }
            } else {
                for (int e = 0; e < 4; ++e)
                    if (i + e >= 0 && i + e < d.n) { const double x = (double)sanitise(ld1(d.g + i + e)); acc += x * x; }
            }
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

// Stage 2: one workgroup adds the partials in a fixed order and writes norm and clip coefficient (clip_grad_norm_'s formula).
__global__ __launch_bounds__(256) void optim_sqnorm_final_kernel(const double* __restrict__ partials, int n_partials, OptimState* __restrict__ state,
                                                                float max_norm) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += 256) acc += partials[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double norm = sqrt(red[0]);
        state->norm = norm;
        const double c = (double)max_norm / (norm + 1e-6);
        state->clip_coef = c < 1.0 ? (float)c : 1.0f;
    }
}

extern "C" int uenc_optim_grad_sqnorm(const void* table, int n, long total_tiles, double* partials, int n_partials, void* state,
                                      float max_norm, hipStream_t stream) {
    UENC_CHECK_ARG(table != nullptr && n > 0 && total_tiles > 0 && partials != nullptr && state != nullptr);
    UENC_CHECK_ARG((((uintptr_t)state) & 15) == 0 && (((uintptr_t)table | (uintptr_t)partials) & 7) == 0 && max_norm > 0.f);
    const int grid = (int)(total_tiles < OPT_MAX_GRID ? total_tiles : OPT_MAX_GRID);
    UENC_CHECK_ARG(n_partials >= grid);
    hipLaunchKernelGGL(optim_sqnorm_partial_kernel, dim3(grid), dim3(256), 0, stream, (const OptimSeg*)table, n, total_tiles, partials);
    hipLaunchKernelGGL(optim_sqnorm_final_kernel, dim3(1), dim3(256), 0, stream, (const double*)partials, grid, (OptimState*)state, max_norm);
    UENC_LAUNCH_RET();
}

// ---- update ----------------------------------------------------------------------------------------------------------------------
struct AdamArgs { float beta2, omb1, omb2, eps; };       // omb = 1 - beta, rounded from the double difference as torch's scalars are

// torch.optim.AdamW (no amsgrad, no maximize) on one element, in torch's order of operations:
//   p *= 1 - lr * wd;  m = lerp(m, g, 1 - beta1);  v = v * beta2 + (1 - beta2) * g * g;
//   p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float coef, float decay, float step_size, float inv_sqrt_bc2,
                                          const AdamArgs& a) {
    g = sanitise(g) * coef;
    p *= decay;
    m = m + a.omb1 * (g - m);
    v = v * a.beta2 + a.omb2 * g * g;
    const float denom = sqrtf(v) * inv_sqrt_bc2 + a.eps;
    p -= step_size * __fdiv_rn(m, denom);
}

__global__ __launch_bounds__(256) void optim_adamw_kernel(const OptimSeg* __restrict__ table, int n, long total_tiles,
                                                          const float4* __restrict__ groups, int n_groups, const OptimState* __restrict__ state,
                                                          AdamArgs a) {
    const float coef = state->clip_coef, inv_bc1 = state->inv_bc1, inv_sqrt_bc2 = state->inv_sqrt_bc2;
    for (long tix = blockIdx.x; tix < total_tiles; tix += gridDim.x) {
        const int s = find_segment(table, n, tix);
        const OptimSeg d = table[s];
        if (d.group < 0 || d.group >= n_groups) continue;
        const float4 hp = groups[d.group];                  // {lr, weight_decay, 1 - lr * weight_decay, unused}
        const float decay = hp.z, step_size = hp.x * inv_bc1;
        const int al = misalign4(d.p);
        const long j0 = (tix - d.tile_begin) * OPT_TILE;
        long idx[4];
        f32x4u P[4], G[4], M[4], V[4];
        bool vec[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {                       // all loads of the tile first: 16 vector loads in flight per lane
            const long i = j0 + k * 1024 + threadIdx.x * 4 - al;
            idx[k] = i;
            vec[k] = i >= 0 && i + 4 <= d.n;
            if (vec[k]) {
                P[k] = ld4(d.p + i); G[k] = ld4(d.g + i);
                M[k] = ld4(d.m + i); V[k] = ld4(d.v + i);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long i = idx[k];
            if (vec[k]) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float p = P[k][e], m = M[k][e], v = V[k][e];
                    adamw_one(p, G[k][e], m, v, coef, decay, step_size, inv_sqrt_bc2, a);
                    P[k][e] = p; M[k][e] = m; V[k][e] = v;
                }
                st4(d.p + i, P[k]); st4(d.m + i, M[k]); st4(d.v + i, V[k]);
            } else {
                for (int e = 0; e < 4; ++e) {
                    const long ie = i + e;
                    if (ie >= 0 && ie < d.n) {
                        float p = ld1(d.p + ie), m = ld1(d.m + ie), v = ld1(d.v + ie);
                        adamw_one(p, ld1(d.g + ie), m, v, coef, decay, step_size, inv_sqrt_bc2, a);
                        st1(d.p + ie, p); st1(d.m + ie, m); st1(d.v + ie, v);
                    }
                }
            }
        }
    }
}

extern "C" int uenc_optim_adamw_step(const void* table, int n, long total_tiles, const float* groups, int n_groups, const void* state,
                                     double beta1, double beta2, double eps, hipStream_t stream) {
    UENC_CHECK_ARG(table != nullptr && n > 0 && total_tiles > 0 && groups != nullptr && n_groups > 0 && state != nullptr);
    UENC_CHECK_ARG((((uintptr_t)state | (uintptr_t)groups) & 15) == 0 && (((uintptr_t)table) & 7) == 0);
    UENC_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0);
    const AdamArgs a = {(float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps};
    const int grid = (int)(total_tiles < OPT_MAX_GRID ? total_tiles : OPT_MAX_GRID);
    hipLaunchKernelGGL(optim_adamw_kernel, dim3(grid), dim3(256), 0, stream, (const OptimSeg*)table, n, total_tiles, (const float4*)groups, n_groups,
                       (const OptimState*)state, a);
    UENC_LAUNCH_RET();
}

// ---- step count ------------------------------------------------------------------------------------------------------------------
// step += 1 on the device (a graph replay advances it by itself), and the bias corrections of the new step in double, as torch's host
// arithmetic has them, rounded once.
__global__ void optim_advance_kernel(OptimState* __restrict__ state, double beta1, double beta2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long t = state->step + 1;
    state->step = t;
    state->inv_bc1 = (float)(1.0 / (1.0 - pow(beta1, (double)t)));
    state->inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow(beta2, (double)t)));
}

extern "C" int uenc_optim_advance(void* state, double beta1, double beta2, hipStream_t stream) {
    UENC_CHECK_ARG(state != nullptr && (((uintptr_t)state) & 15) == 0);
    UENC_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0);
    hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(64), 0, stream, (OptimState*)state, beta1, beta2);
    UENC_LAUNCH_RET();
}
