// Query-tiled multi-head attention core (head_dim 32, unmasked), forward and backward (gfx950).
//
// The core of nn.MultiheadAttention when a whole feature map attends to itself -- the DETR encoder of
// TransformerEncoderPixelDecoder on res5 (modeling/pixel_decoder/fpn.py, transformer.py:161-234): thousands of queries against as
// many keys.  csrc/mha.hip is built for <= 160 queries per slice and holds every query in LDS in its dK / dV kernel (Lq <= 960);
// here nothing but the grid bounds Lq or S.
//
// Tensor contract of uenc_mha_fwd / uenc_mha_bwd without the mask and the workspace: q (B, Lq, *) / k, v (B, S, *) bf16, heads
// interleaved in the row (head h at columns 32h..32h+31), arbitrary 16-byte aligned row / batch strides; lse (B, H, Lq) in the log2
// domain; dropout on the probabilities by attn_keep() with element index ((b H + h) Lq + q) S + key.
//
// Tiles: TQ = 64 queries per workgroup (forward, dQ), TK = 64 keys per LDS block and per workgroup (dK / dV).  One workgroup =
// 4 waves, one wave = one 16-row MFMA tile of its workgroup's 64 rows.
//   forward / dQ : grid = ceil(Lq / 64) * B * H workgroups; a wave keeps its Q (and dO) fragment in registers and sweeps the keys
//                  through double-buffered 64-key LDS blocks of K and V (S^T = K Q^T: a lane owns one query column, online softmax
//                  in registers, P^T / dS^T feed the second MFMA from registers).  dQ is WRITTEN (fp32), not accumulated.
//   dK / dV      : grid = ceil(S / 64) * B * H workgroups; a wave keeps its K and V fragment and the dK / dV accumulators in
//                  registers and sweeps the queries through double-buffered 64-query LDS blocks of Q, dO, lse and delta (delta =
//                  sum_d out dO is formed while the block is staged: 4 lanes per row).
// No atomics, no zeroed outputs: every output element has one writer and one summation order, so two runs give the same bits.
// Workload shape (B H = 16, Lq = S = 2048): 32 * 16 = 512 workgroups in each of the three kernels, two per CU on 256 CUs.
// The 1-D grid is decoded (tile fastest, then image * H + head) behind xcd_remap, so the tiles of one (image, head) -- which stream
// the same K / V or Q / dO rows -- run on one XCD and share its L2.
//
// Rounding points (those of csrc/mha.hip): P to bf16 in front of P V, the bf16 out reused for delta, dS to bf16 in front of both
// gradient products, bf16 dk / dv, fp32 dq.
// Algorithmic HBM bytes per (image, head): forward (Lq + 2 S) * 64 + Lq * 64; K / V re-reads by the Lq / 64 query tiles are L2 traffic.
#include "common.h"
#include "lds_frag.h"

#define LOG2E 1.4426950408889634f
__device__ __forceinline__ float at_vmaxf(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float at_vmax3f(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
#define NEG_INF (-__builtin_huge_valf())
#define TQ 64             // queries per workgroup (forward, dQ) and per LDS block (dK / dV)
#define TK 64             // keys per LDS block (forward, dQ) and per workgroup (dK / dV)

struct AtP {
    const bf16 *q, *k, *v;
    long q_bs, q_rs, k_bs, k_rs, v_bs, v_rs;       // batch / row strides in elements
    bf16* out; long o_bs, o_rs;                     // (B, Lq, *)
    float* lse;                                     // (B, H, Lq) log2-domain log-sum-exp
    const bf16* dout; long do_bs, do_rs;
    float* dq;  long dq_bs, dq_rs;                  // fp32, written
    bf16 *dk, *dv; long dk_bs, dk_rs, dv_bs, dv_rs;
    int B, H, Lq, S, nqt, nkt;
    float scale;
    unsigned drop_thresh, seed;                     // attention-probability dropout (0 = off): attn_keep() of common.h
    const unsigned* seed_ptr;                       // non-NULL: the seed is read from this device word instead (the *_sp entries)
    float inv_keep;
};

// ------------------------------------------------------------------------------------------------
// forward (MODE 0) and dQ (MODE 1): a workgroup owns 64 queries, a wave 16 of them; loop over all keys
// ------------------------------------------------------------------------------------------------
template <int MODE, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_tiled_q_kernel(AtP p) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * TK * 64];
    unsigned char* Ks = smem;                            // 2 stages x 64 rows
    unsigned char* Vs = smem + 2 * TK * 64;

    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int qt = lb % p.nqt, bh = lb / p.nqt;
    const unsigned seed = DROP ? (p.seed_ptr != nullptr ? *p.seed_ptr : p.seed) : 0u;
    const int b = bh / p.H, h = bh - b * p.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fg = lane >> 4;
    const int nblk = (p.S + TK - 1) / TK;
    const bf16* kb = p.k + b * p.k_bs + h * 32;
    const bf16* vb = p.v + b * p.v_bs + h * 32;
    const int qidx = qt * TQ + wave * 16 + fr;           // this lane's query (column of S^T)
    const bool active = qt * TQ + wave * 16 < p.Lq;      // wave-uniform: the wave's tile has a row

    // K / V block staging: one 16-byte chunk of each per thread
    const int srow = threadIdx.x >> 2, sch = threadIdx.x & 3;
    u32x4 rk, rv;
    auto gload = [&](int blk) {
        const int key = blk * TK + srow;
        rk = (u32x4){0u, 0u, 0u, 0u}; rv = rk;
        if (key < p.S) {
            rk = *(const u32x4*)(kb + (long)key * p.k_rs + sch * 8);
            rv = *(const u32x4*)(vb + (long)key * p.v_rs + sch * 8);
        }
    };
    auto lstore = [&](int st) {
        *(u32x4*)(Ks + st * TK * 64 + rm_off(srow, sch)) = rk;
        *(u32x4*)(Vs + st * TK * 64 + rm_off(srow, sch)) = rv;
    };
    gload(0); lstore(0);

    // the wave's Q (and dO) fragment, straight from memory: lane = (row fr, columns 8 fg ..); rows past Lq are zero
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const float sc = p.scale * LOG2E;
    bf16x8 qf, dof;
#pragma unroll
    for (int j = 0; j < 8; ++j) { qf[j] = (bf16)0.f; dof[j] = (bf16)0.f; }
    float m_run = -1e30f, l_run = 0.f, lse_q = 0.f, dl_q = 0.f;
    f32x4 o[2] = {zero4, zero4};
    if (qidx < p.Lq) {
        qf = *(const bf16x8*)(p.q + b * p.q_bs + (long)qidx * p.q_rs + h * 32 + 8 * fg);
        if (MODE == 1) {
            dof = *(const bf16x8*)(p.dout + b * p.do_bs + (long)qidx * p.do_rs + h * 32 + 8 * fg);
            const bf16x8 ov = *(const bf16x8*)(p.out + b * p.o_bs + (long)qidx * p.o_rs + h * 32 + 8 * fg);
#pragma unroll
            for (int j = 0; j < 8; ++j) dl_q += (float)ov[j] * (float)dof[j];
            lse_q = p.lse[((long)b * p.H + h) * p.Lq + qidx];
        }
    }
    if (MODE == 1) {
        dl_q = xor16_sum(dl_q);
        dl_q = xor32_sum(dl_q);
    }
    __syncthreads();

    for (int blk = 0; blk < nblk; ++blk) {
        const int st = blk & 1;
        if (blk + 1 < nblk) gload(blk + 1);
        const unsigned char* Kc = Ks + st * TK * 64;
        const unsigned char* Vc = Vs + st * TK * 64;
        const int kbase = blk * TK;
        if (active) {
            f32x4 s[4];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) s[kt] = mfma16(frag_rows(Kc, kt * 16, fr, fg), qf, zero4);
            float v[4][4];                              // (a copy in plain registers: the MFMA results live in accumulation registers)
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[kt][r] = s[kt][r];
            if (kbase + TK > p.S) {                     // the ragged last block: keys past the end score -inf (exp2 -> 0)
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[kt][r] = (kbase + kt * 16 + 4 * fg + r < p.S) ? v[kt][r] : NEG_INF;
            }
            if (MODE == 0) {
                float mloc = at_vmax3f(v[0][0], v[0][1], v[0][2]);
                mloc = at_vmax3f(mloc, v[0][3], v[1][0]); mloc = at_vmax3f(mloc, v[1][1], v[1][2]); mloc = at_vmax3f(mloc, v[1][3], v[2][0]);
                mloc = at_vmax3f(mloc, v[2][1], v[2][2]); mloc = at_vmax3f(mloc, v[2][3], v[3][0]); mloc = at_vmax3f(mloc, v[3][1], v[3][2]);
                mloc = at_vmaxf(mloc, v[3][3]);
                mloc = xor16_max(mloc);
                mloc = xor32_max(mloc);
                const float mnew = at_vmaxf(m_run, mloc * sc);       // (every block holds at least one key < S)
                const float alpha = fast_exp2(m_run - mnew);
                const float nm = -mnew;
                float sum = 0.f;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float e = fast_exp2(__builtin_fmaf(v[kt][r], sc, nm));
                        sum += e;                                    // the softmax normaliser is taken BEFORE dropout
                        v[kt][r] = e;
                        if (DROP)
                            v[kt][r] = attn_keep(seed, p.drop_thresh, ((unsigned long long)bh * p.Lq + qidx) * p.S + (kbase + kt * 16 + 4 * fg + r))
                                           ? e * p.inv_keep : 0.f;
                    }
                sum = xor16_sum(sum);
                sum = xor32_sum(sum);
                l_run = l_run * alpha + sum;
                m_run = mnew;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
#pragma unroll
                for (int kb2 = 0; kb2 < 2; ++kb2) {
                    bf16x8 pb;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { pb[r] = (bf16)v[2 * kb2][r]; pb[4 + r] = (bf16)v[2 * kb2 + 1][r]; }
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
                        o[dt] = mfma16(frag_tr(Vc, 32 * kb2, 32 * kb2 + 16, dt * 16, lane), pb, o[dt]);
                }
            } else {
                // dS^T = P * (dP^T - delta), P from the saved log-sum-exp; dQ^T += K^T dS^T
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    const f32x4 dp = mfma16(frag_rows(Vc, kt * 16, fr, fg), dof, zero4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float pr = fast_exp2(__builtin_fmaf(v[kt][r], sc, -lse_q));
                        float dpv = dp[r];
                        if (DROP)
                            dpv = attn_keep(seed, p.drop_thresh, ((unsigned long long)bh * p.Lq + qidx) * p.S + (kbase + kt * 16 + 4 * fg + r))
                                      ? dpv * p.inv_keep : 0.f;
                        v[kt][r] = pr * (dpv - dl_q);
                    }
                }
#pragma unroll
                for (int kb2 = 0; kb2 < 2; ++kb2) {
                    bf16x8 pb;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { pb[r] = (bf16)v[2 * kb2][r]; pb[4 + r] = (bf16)v[2 * kb2 + 1][r]; }
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
                        o[dt] = mfma16(frag_tr(Kc, 32 * kb2, 32 * kb2 + 16, dt * 16, lane), pb, o[dt]);
                }
            }
        }
        if (blk + 1 < nblk) lstore(st ^ 1);
        __syncthreads();
    }

    if (qidx >= p.Lq) return;
    if (MODE == 1) {
        float* dst = p.dq + b * p.dq_bs + (long)qidx * p.dq_rs + h * 32;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            f32x4 g;
#pragma unroll
            for (int r = 0; r < 4; ++r) g[r] = o[dt][r] * p.scale;
            *(f32x4*)(dst + dt * 16 + 4 * fg) = g;
        }
    } else {
        const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            bf16x4 ov;
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[r] = (bf16)(o[dt][r] * inv);
            *(bf16x4*)(p.out + b * p.o_bs + (long)qidx * p.o_rs + h * 32 + dt * 16 + 4 * fg) = ov;
        }
        if (fg == 0 && p.lse != nullptr) p.lse[((long)b * p.H + h) * p.Lq + qidx] = m_run + log2f(fmaxf(l_run, 1e-37f));
    }
}

// ------------------------------------------------------------------------------------------------
// dK / dV: a workgroup owns 64 keys, a wave 16 of them; loop over all queries
// ------------------------------------------------------------------------------------------------
template <bool DROP>
__global__ __launch_bounds__(256, 2) void attn_tiled_dkdv_kernel(AtP p) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * TQ * 64 + 4 * TQ * 4];
    unsigned char* Qs = smem;                            // 2 stages x 64 rows
    unsigned char* dOs = smem + 2 * TQ * 64;
    float* lse_s = (float*)(smem + 4 * TQ * 64);         // 2 stages x 64
    float* dl_s = lse_s + 2 * TQ;

    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int ktile = lb % p.nkt, bh = lb / p.nkt;
    const unsigned seed = DROP ? (p.seed_ptr != nullptr ? *p.seed_ptr : p.seed) : 0u;
    const int b = bh / p.H, h = bh - b * p.H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fg = lane >> 4;
    const int nblk = (p.Lq + TQ - 1) / TQ;
    const int key = ktile * TK + wave * 16 + fr;         // this lane's key (column)
    const bool active = ktile * TK + wave * 16 < p.S;    // wave-uniform
    const bf16* qb = p.q + b * p.q_bs + h * 32;
    const bf16* gb = p.dout + b * p.do_bs + h * 32;
    const bf16* ob = p.out + b * p.o_bs + h * 32;
    const float* lrow = p.lse + ((long)b * p.H + h) * p.Lq;

    // Q / dO block staging: one 16-byte chunk of each per thread; the four lanes of a row form delta = sum_d out dO on the way
    const int srow = threadIdx.x >> 2, sch = threadIdx.x & 3;
    u32x4 rq, rg;
    float rl, rd;
    auto gload = [&](int blk) {
        const int qi = blk * TQ + srow;
        rq = (u32x4){0u, 0u, 0u, 0u}; rg = rq; rl = 0.f;
        float part = 0.f;
        if (qi < p.Lq) {
            rq = *(const u32x4*)(qb + (long)qi * p.q_rs + sch * 8);
            const bf16x8 gv = *(const bf16x8*)(gb + (long)qi * p.do_rs + sch * 8);
            const bf16x8 ov = *(const bf16x8*)(ob + (long)qi * p.o_rs + sch * 8);
            rg = __builtin_bit_cast(u32x4, gv);
#pragma unroll
            for (int j = 0; j < 8; ++j) part += (float)ov[j] * (float)gv[j];
            rl = lrow[qi];
        }
        part = dpp_add_f32<0xB1>(part);                  // quad_perm [1,0,3,2]
        rd = dpp_add_f32<0x4E>(part);                    // quad_perm [2,3,0,1]: the row's four chunks
    };
    auto lstore = [&](int st) {
        *(u32x4*)(Qs + st * TQ * 64 + rm_off(srow, sch)) = rq;
        *(u32x4*)(dOs + st * TQ * 64 + rm_off(srow, sch)) = rg;
        if (sch == 0) { lse_s[st * TQ + srow] = rl; dl_s[st * TQ + srow] = rd; }
    };
    gload(0); lstore(0);

    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const float sc = p.scale * LOG2E;
    bf16x8 kfB, vfB;
#pragma unroll
    for (int j = 0; j < 8; ++j) { kfB[j] = (bf16)0.f; vfB[j] = (bf16)0.f; }
    if (key < p.S) {
        kfB = *(const bf16x8*)(p.k + b * p.k_bs + (long)key * p.k_rs + h * 32 + 8 * fg);
        vfB = *(const bf16x8*)(p.v + b * p.v_bs + (long)key * p.v_rs + h * 32 + 8 * fg);
    }
    f32x4 dk[2] = {zero4, zero4}, dv[2] = {zero4, zero4};
    __syncthreads();

    for (int blk = 0; blk < nblk; ++blk) {
        const int st = blk & 1;
        if (blk + 1 < nblk) gload(blk + 1);
        const unsigned char* Qc = Qs + st * TQ * 64;
        const unsigned char* Gc = dOs + st * TQ * 64;
        const float* lc = lse_s + st * TQ;
        const float* dc = dl_s + st * TQ;
        if (active) {
#pragma unroll
            for (int qb2 = 0; qb2 < TQ / 32; ++qb2) {
                if (blk * TQ + 32 * qb2 >= p.Lq) break;             // nothing but padding rows from here on
                f32x4 pt[2], dst[2];
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const int qt = 2 * qb2 + h2;
                    const f32x4 sv = mfma16(frag_rows(Qc, qt * 16, fr, fg), kfB, zero4);       // S[q = 4fg + r][key = fr]
                    const f32x4 dp = mfma16(frag_rows(Gc, qt * 16, fr, fg), vfB, zero4);
                    const float4 l4 = *(const float4*)(lc + qt * 16 + 4 * fg);
                    const float4 d4 = *(const float4*)(dc + qt * 16 + 4 * fg);
                    const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv4[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int qi = blk * TQ + qt * 16 + 4 * fg + r;
                        // (no validity tests: a padding query has zero Q / dO rows and lse = delta = 0 -> p = 1, dS = 0, and P^T dO adds
                        // nothing; a key past the end only feeds its own column, which is never stored)
                        const float pr = fast_exp2(__builtin_fmaf(sv[r], sc, -lv[r]));
                        float keepw = 1.0f;
                        if (DROP && (key < p.S) && (qi < p.Lq))
                            keepw = attn_keep(seed, p.drop_thresh, ((unsigned long long)bh * p.Lq + qi) * p.S + key) ? p.inv_keep : 0.f;
                        pt[h2][r] = pr * keepw;
                        dst[h2][r] = pr * (dp[r] * keepw - dv4[r]);
                    }
                }
                bf16x8 pb, db;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pb[r] = (bf16)pt[0][r]; pb[4 + r] = (bf16)pt[1][r];
                    db[r] = (bf16)dst[0][r]; db[4 + r] = (bf16)dst[1][r];
                }
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    dv[dt] = mfma16(frag_tr(Gc, 32 * qb2, 32 * qb2 + 16, dt * 16, lane), pb, dv[dt]);
                    dk[dt] = mfma16(frag_tr(Qc, 32 * qb2, 32 * qb2 + 16, dt * 16, lane), db, dk[dt]);
                }
            }
        }
        if (blk + 1 < nblk) lstore(st ^ 1);
        __syncthreads();
    }

    if (key < p.S) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            bf16x4 kv, vv;
#pragma unroll
            for (int r = 0; r < 4; ++r) { kv[r] = (bf16)(dk[dt][r] * p.scale); vv[r] = (bf16)dv[dt][r]; }
            *(bf16x4*)(p.dk + b * p.dk_bs + (long)key * p.dk_rs + h * 32 + dt * 16 + 4 * fg) = kv;
            *(bf16x4*)(p.dv + b * p.dv_bs + (long)key * p.dv_rs + h * 32 + dt * 16 + 4 * fg) = vv;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// which = 0: queries per workgroup of the forward / dQ kernel; 1: keys per LDS block and per workgroup of the dK / dV kernel
extern "C" int uenc_attn_tiled_tile(int which) { return which == 0 ? TQ : (which == 1 ? TK : UENC_EINVAL); }

static int at_fill(AtP& p, const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs, long v_rs,
                   int B, int H, int Lq, int S, float scale, float dropout_p, unsigned seed, const unsigned* seed_ptr) {
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return UENC_EINVAL;
    p.drop_thresh = attn_drop_thresh(dropout_p); p.seed = seed; p.seed_ptr = seed_ptr; p.inv_keep = 1.0f / (1.0f - dropout_p);
    if (!(q && k && v && B > 0 && H > 0 && Lq > 0 && S > 0)) return UENC_EINVAL;
    if ((q_rs | k_rs | v_rs | q_bs | k_bs | v_bs) & 7) return UENC_EINVAL;                   // 16-byte rows
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) return UENC_EINVAL;
    p.nqt = (Lq + TQ - 1) / TQ; p.nkt = (S + TK - 1) / TK;
    if ((long)p.nqt * B * H > 0x7fffffffL || (long)p.nkt * B * H > 0x7fffffffL) return UENC_EINVAL;   // the 1-D grids
    p.q = (const bf16*)q; p.k = (const bf16*)k; p.v = (const bf16*)v;
    p.q_bs = q_bs; p.q_rs = q_rs; p.k_bs = k_bs; p.k_rs = k_rs; p.v_bs = v_bs; p.v_rs = v_rs;
    p.B = B; p.H = H; p.Lq = Lq; p.S = S; p.scale = scale;
    p.out = nullptr; p.lse = nullptr; p.dout = nullptr; p.dq = nullptr; p.dk = p.dv = nullptr;
    return UENC_OK;
}

// out (B, Lq, *) bf16, 8-byte aligned rows; lse (B, H, Lq) fp32 (needed by the backward; may be NULL).
static int at_fwd_impl(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs, long v_rs,
                       void* out, long o_bs, long o_rs, float* lse, int B, int H, int Lq, int S, float scale, float dropout_p,
                       unsigned seed, const unsigned* seed_ptr, hipStream_t stream) {
    AtP p;
    int rc = at_fill(p, q, q_bs, q_rs, k, k_bs, k_rs, v, v_bs, v_rs, B, H, Lq, S, scale, dropout_p, seed, seed_ptr);
    if (rc != UENC_OK) return rc;
    UENC_CHECK_ARG(out && ((o_rs | o_bs) & 3) == 0 && ((uintptr_t)out & 7) == 0);
    p.out = (bf16*)out; p.o_bs = o_bs; p.o_rs = o_rs; p.lse = lse;
    const dim3 grid((unsigned)(p.nqt * B * H));
    if (p.drop_thresh != 0u) hipLaunchKernelGGL((attn_tiled_q_kernel<0, true>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((attn_tiled_q_kernel<0, false>), grid, dim3(256), 0, stream, p);
    UENC_LAUNCH_RET();
}

// dq (B, Lq, *) fp32 WRITTEN, 16-byte aligned rows; dk, dv (B, S, *) bf16 written for every key and head, 8-byte aligned rows.
static int at_bwd_impl(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs, long v_rs,
                       const void* out, long o_bs, long o_rs, const float* lse, const void* dout, long do_bs, long do_rs, float* dq,
                       long dq_bs, long dq_rs, void* dk, long dk_bs, long dk_rs, void* dv, long dv_bs, long dv_rs, int B, int H, int Lq,
                       int S, float scale, float dropout_p, unsigned seed, const unsigned* seed_ptr, hipStream_t stream) {
    AtP p;
    int rc = at_fill(p, q, q_bs, q_rs, k, k_bs, k_rs, v, v_bs, v_rs, B, H, Lq, S, scale, dropout_p, seed, seed_ptr);
    if (rc != UENC_OK) return rc;
    UENC_CHECK_ARG(out && lse && dout && dq && dk && dv);
    UENC_CHECK_ARG(((o_rs | do_rs | o_bs | do_bs) & 7) == 0 && (((uintptr_t)out | (uintptr_t)dout) & 15) == 0);
    UENC_CHECK_ARG(((dq_rs | dq_bs) & 3) == 0 && ((uintptr_t)dq & 15) == 0);
    UENC_CHECK_ARG(((dk_rs | dv_rs | dk_bs | dv_bs) & 3) == 0 && (((uintptr_t)dk | (uintptr_t)dv) & 7) == 0);
    p.out = (bf16*)out; p.o_bs = o_bs; p.o_rs = o_rs; p.lse = (float*)lse;
    p.dout = (const bf16*)dout; p.do_bs = do_bs; p.do_rs = do_rs;
    p.dq = dq; p.dq_bs = dq_bs; p.dq_rs = dq_rs;
    p.dk = (bf16*)dk; p.dk_bs = dk_bs; p.dk_rs = dk_rs; p.dv = (bf16*)dv; p.dv_bs = dv_bs; p.dv_rs = dv_rs;
    const dim3 gq((unsigned)(p.nqt * B * H)), gk((unsigned)(p.nkt * B * H));
    if (p.drop_thresh != 0u) {
        hipLaunchKernelGGL((attn_tiled_q_kernel<1, true>), gq, dim3(256), 0, stream, p);
        hipLaunchKernelGGL(attn_tiled_dkdv_kernel<true>, gk, dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL((attn_tiled_q_kernel<1, false>), gq, dim3(256), 0, stream, p);
        hipLaunchKernelGGL(attn_tiled_dkdv_kernel<false>, gk, dim3(256), 0, stream, p);
    }
    UENC_LAUNCH_RET();
}

extern "C" int uenc_attn_tiled_fwd(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs,
                                   long v_rs, void* out, long o_bs, long o_rs, float* lse, int B, int H, int Lq, int S, float scale,
                                   float dropout_p, unsigned seed, hipStream_t stream) {
    return at_fwd_impl(q, q_bs, q_rs, k, k_bs, k_rs, v, v_bs, v_rs, out, o_bs, o_rs, lse, B, H, Lq, S, scale, dropout_p, seed, nullptr, stream);
}

extern "C" int uenc_attn_tiled_bwd(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs,
                                   long v_rs, const void* out, long o_bs, long o_rs, const float* lse, const void* dout, long do_bs,
                                   long do_rs, float* dq, long dq_bs, long dq_rs, void* dk, long dk_bs, long dk_rs, void* dv, long dv_bs,
                                   long dv_rs, int B, int H, int Lq, int S, float scale, float dropout_p, unsigned seed,
                                   hipStream_t stream) {
    return at_bwd_impl(q, q_bs, q_rs, k, k_bs, k_rs, v, v_bs, v_rs, out, o_bs, o_rs, lse, dout, do_bs, do_rs, dq, dq_bs, dq_rs, dk, dk_bs,
                       dk_rs, dv, dv_bs, dv_rs, B, H, Lq, S, scale, dropout_p, seed, nullptr, stream);
}

// Seed-by-pointer twins (HIP-graph capture): the dropout seed is seeds[slot], read by the kernels themselves.  Same arithmetic.
extern "C" int uenc_attn_tiled_fwd_sp(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs,
                                      long v_rs, void* out, long o_bs, long o_rs, float* lse, int B, int H, int Lq, int S, float scale,
                                      float dropout_p, const unsigned* seeds, int slot, hipStream_t stream) {
    UENC_CHECK_ARG(seeds != nullptr && slot >= 0);
    return at_fwd_impl(q, q_bs, q_rs, k, k_bs, k_rs, v, v_bs, v_rs, out, o_bs, o_rs, lse, B, H, Lq, S, scale, dropout_p, 0u, seeds + slot,
                       stream);
}

extern "C" int uenc_attn_tiled_bwd_sp(const void* q, long q_bs, long q_rs, const void* k, long k_bs, long k_rs, const void* v, long v_bs,
                                      long v_rs, const void* out, long o_bs, long o_rs, const float* lse, const void* dout, long do_bs,
                                      long do_rs, float* dq, long dq_bs, long dq_rs, void* dk, long dk_bs, long dk_rs, void* dv,
                                      long dv_bs, long dv_rs, int B, int H, int Lq, int S, float scale, float dropout_p,
                                      const unsigned* seeds, int slot, hipStream_t stream) {
    UENC_CHECK_ARG(seeds != nullptr && slot >= 0);
    return at_bwd_impl(q, q_bs, q_rs, k, k_bs, k_rs, v, v_bs, v_rs, out, o_bs, o_rs, lse, dout, do_bs, do_rs, dq, dq_bs, dq_rs, dk, dk_bs,
                       dk_rs, dv, dv_bs, dv_rs, B, H, Lq, S, scale, dropout_p, 0u, seeds + slot, stream);
}
