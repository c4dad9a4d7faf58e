// Device-side per-step randomness (ops.device_rng): the prerequisite for capturing a training step once and replaying it as a HIP graph.
//
// A replayed graph repeats its kernel arguments verbatim, so nothing random may be decided on the host.  Instead:
//   * uenc_step_rng_advance reads a device state (64-bit base seed, 64-bit step counter), increments the counter itself and writes
//       - the per-sample DropPath multipliers of every registered branch slot: keep ? 1 / keep_prob : 0,
//       - one 32-bit dropout seed per registered seed slot;
//   * the DropPath GEMMs read their multipliers through the existing sample_scale pointers, the dropout kernels read seeds[slot].
// Both tables are pure functions of (base seed, step, slot, sample) built from uenc_mix32 (the attn_keep hash of common.h), so the host
// can restate them exactly (uenc.kernels.step_rng_reference).
#include "common.h"

// Tag bits that keep the index spaces of the two tables apart.
#define STEP_RNG_SEED_TAG (1ull << 40)
#define STEP_RNG_DP_TAG (1ull << 41)

__device__ __forceinline__ unsigned step_key(unsigned long long base, unsigned long long step) {
    const unsigned h = uenc_mix32((unsigned)(base >> 32), step);
    return uenc_mix32((unsigned)base ^ h, step);
}

// One workgroup: every lane reads the state before the barrier, lane 0 writes the incremented counter after it.
__global__ __launch_bounds__(256) void step_rng_advance_kernel(unsigned long long* __restrict__ state, const float* __restrict__ keep_prob,
                                                               int n_branch, int n_samples, float* __restrict__ scales, int n_seed,
                                                               unsigned* __restrict__ seeds, int advance) {
    const unsigned long long base = state[0];
    const unsigned long long step = state[1] + (advance ? 1ull : 0ull);
    __syncthreads();
    if (threadIdx.x == 0 && advance) state[1] = step;
    const unsigned key = step_key(base, step);
    for (int i = threadIdx.x; i < n_seed; i += 256) seeds[i] = uenc_mix32(key, STEP_RNG_SEED_TAG | (unsigned long long)i);
    const long nb = (long)n_branch * n_samples;
    for (long i = threadIdx.x; i < nb; i += 256) {
        const float kp = keep_prob[i / n_samples];
        const float dp = 1.0f - kp;                                   // the drop probability, thresholded as attn_drop_thresh does
        const unsigned thresh = dp <= 0.f ? 0u : (dp >= 1.f ? 0xffffffffu : (unsigned)((double)dp * 4294967296.0));
        const bool keep = kp > 0.f && uenc_mix32(key, STEP_RNG_DP_TAG | (unsigned long long)i) >= thresh;
        scales[i] = keep ? __fdiv_rn(1.0f, kp) : 0.0f;
    }
}

extern "C" int uenc_step_rng_advance(unsigned long long* state, const float* keep_prob, int n_branch, int n_samples, float* scales,
                                     int n_seed, unsigned* seeds, int advance, hipStream_t stream) {
    UENC_CHECK_ARG(state != nullptr && n_branch >= 0 && n_seed >= 0 && n_samples > 0);
    UENC_CHECK_ARG(n_branch == 0 || (keep_prob != nullptr && scales != nullptr));
    UENC_CHECK_ARG(n_seed == 0 || seeds != nullptr);
    hipLaunchKernelGGL(step_rng_advance_kernel, dim3(1), dim3(256), 0, stream, state, keep_prob, n_branch, n_samples, scales, n_seed, seeds,
                       advance);
    UENC_LAUNCH_RET();
}

// Inverted dropout with the seed read from seeds[slot]: out[i] = keep(i) ? in[i] / (1 - p) : 0 with keep(i) = attn_keep(seed, thresh, i)
// -- for bf16 the arithmetic of uenc_dropout_bf16 (bit-identical for the same seed), for fp32 the same mask on fp32 data.  Any n; in
// place allowed.
template <typename T>
__global__ __launch_bounds__(256) void dropout_sp_kernel(const T* __restrict__ in, T* __restrict__ out, long n, const unsigned* __restrict__ seeds,
                                                         int slot, unsigned thresh, float inv_keep) {
    const unsigned seed = seeds[slot];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        out[i] = attn_keep(seed, thresh, (unsigned long long)i) ? (T)((float)in[i] * inv_keep) : (T)0.f;
}

__global__ __launch_bounds__(256) void dropout_sp_bf16x8_kernel(const bf16* __restrict__ in, bf16* __restrict__ out, long n8,
                                                                const unsigned* __restrict__ seeds, int slot, unsigned thresh, float inv_keep) {
    const unsigned seed = seeds[slot];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        const bf16x8 v = *(const bf16x8*)(in + i * 8);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = attn_keep(seed, thresh, (unsigned long long)(i * 8 + j)) ? (bf16)((float)v[j] * inv_keep) : (bf16)0.f;
        *(bf16x8*)(out + i * 8) = o;
    }
}

extern "C" int uenc_dropout_sp(const void* in, void* out, long n, int dtype, const unsigned* seeds, int slot, float p, hipStream_t stream) {
    UENC_CHECK_ARG(in && out && seeds && slot >= 0 && n > 0 && p >= 0.f && p < 1.f);
    UENC_CHECK_ARG(dtype == UENC_F32 || dtype == UENC_BF16);
    const unsigned thresh = attn_drop_thresh(p);
    const float inv_keep = 1.0f / (1.0f - p);
    if (dtype == UENC_BF16 && n % 8 == 0 && ((((uintptr_t)in | (uintptr_t)out) & 15) == 0)) {
        long blocks = (n / 8 + 255) / 256;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(dropout_sp_bf16x8_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const bf16*)in, (bf16*)out, n / 8, seeds,
                           slot, thresh, inv_keep);
        UENC_LAUNCH_RET();
    }
    long blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (dtype == UENC_BF16)
        hipLaunchKernelGGL(dropout_sp_kernel<bf16>, dim3((unsigned)blocks), dim3(256), 0, stream, (const bf16*)in, (bf16*)out, n, seeds, slot,
                           thresh, inv_keep);
    else
        hipLaunchKernelGGL(dropout_sp_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, stream, (const float*)in, (float*)out, n, seeds,
                           slot, thresh, inv_keep);
    UENC_LAUNCH_RET();
}

// out[r][c] = bf16(in[r][c] * sample_scale[r / rows_per_sample]): the DropPath-scaled gradient rows that the weight-gradient GEMM of a
// branch reads when its per-sample multipliers live on the device (a replayable step cannot choose row ranges on the host).  C % 8 == 0.
__global__ __launch_bounds__(256) void scale_rows_bf16_kernel(const bf16* __restrict__ in, long ld_in, bf16* __restrict__ out, long ld_out,
                                                              long M, int C8, const float* __restrict__ sample_scale, long rows_per_sample) {
    const long n = M * C8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long r = i / C8, c = (i - r * C8) * 8;
        const float s = sample_scale[r / rows_per_sample];
        const bf16x8 v = *(const bf16x8*)(in + r * ld_in + c);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)v[j] * s);
        *(bf16x8*)(out + r * ld_out + c) = o;
    }
}

extern "C" int uenc_scale_rows_bf16(const void* in, long ld_in, void* out, long ld_out, long M, int C, const float* sample_scale,
                                    long rows_per_sample, hipStream_t stream) {
    UENC_CHECK_ARG(in && out && sample_scale && M > 0 && C > 0 && C % 8 == 0 && rows_per_sample > 0 && M % rows_per_sample == 0);
    UENC_CHECK_ARG(ld_in >= C && ld_out >= C && ld_in % 8 == 0 && ld_out % 8 == 0 && ((((uintptr_t)in | (uintptr_t)out) & 15) == 0));
    long blocks = (M * (C / 8) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(scale_rows_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const bf16*)in, ld_in, (bf16*)out, ld_out, M, C / 8,
                       sample_scale, rows_per_sample);
    UENC_LAUNCH_RET();
}

// Stream-ordered copy of a descriptor table from pinned host memory: the copy a captured step records, so that a replay re-reads the
// table from a host buffer the captured step owns (torch's pinned-tensor copies record allocator events, which a capture must not).
extern "C" int uenc_upload(void* dst, const void* src, long bytes, hipStream_t stream) {
    UENC_CHECK_ARG(dst && src && bytes > 0);
    const hipError_t e = hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, stream);
    return e == hipSuccess ? UENC_OK : (int)e;
}
