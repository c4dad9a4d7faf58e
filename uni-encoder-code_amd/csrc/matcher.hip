// Bipartite matching of predictions to ground-truth segments (uenc.modeling.matcher.HungarianMatcher; reference model/modeling/matcher.py):
// the matching cost of HungarianMatcher.memory_efficient_forward (matcher.py:126-171) and the linear sum assignment scipy solves for it
// (matcher.py:19-36, 173), for a batch of independent problems (problem = one prediction head of one image), with nothing read back.
//
//   uenc_match_cost   C[q][t] = w_mask * cost_mask + w_class * cost_class + w_dice * cost_dice, NaN -> nan_fill (100), in two launches:
//     match_cost_partial_kernel   grid (S point splits, 64 x 64 output tiles, problems).  Per tile of 64 points a workgroup samples its 64
//                                 mask logits x and its 64 targets t bilinearly (grid_sample at 2p - 1, align_corners = False, zero padding)
//                                 into LDS -- x, sigmoid(x) and t never reach HBM -- and adds the two contractions x.t and sigmoid(x).t on
//                                 the VALU in fp32, 4 x 4 outputs per lane; the row sums of softplus(x), sigmoid(x) and the column sum of
//                                 t fall out of the sampling.  softplus(x) - softplus(-x) = x, so
//                                     cost_mask * P = sum_k softplus(x) - sum_k x t.
//                                 Each split writes its partial sums to the workspace: no atomics, the same input gives the same bits.
//     match_cost_finish_kernel    grid (Q, problems), one wave per row: adds the S partials in split order (double), the softmax of the
//                                 class logits, combines the three terms in the reference's order and writes row q of C.
//   uenc_lsap_solve   shortest augmenting paths (Jonker-Volgenant as scipy's rectangular_lsap implements it), one workgroup per problem,
//                     one lane per column, duals and path costs in double, the per-step column minimum as a wave + workgroup reduction.
//
// The problem descriptors are HOST arrays: the entry points copy them into the kernel arguments (at most 32 / 64 problems per launch), so
// there is no device table to upload and a stream capture records the pointers by value like any other launch.
#include "common.h"

#define MC_PT 64                  // points per tile
#define MC_TILE 64                // queries x targets per workgroup
#define MC_MAX_SPLIT 16
#define MC_MAX_PROB 32            // problems per launch (48-byte descriptors in the kernel arguments)
#define LSAP_MAX_N 256
#define LSAP_MAX_PROB 64
#define LSAP_LDS_ENTRIES 10240    // cost matrices up to this many entries are staged in LDS (40 KB); larger ones are read from L2

struct MatchProb {
    const float* logits;          // (Q, C1) class logits of this head and image
    const float* masks;           // (Q, h, w) mask logits
    const float* points;          // (P, 2) x, y in [0, 1]
    const unsigned char* gt;      // (T, Hg, Wg) 0 / 1
    const long long* labels;      // (T)
    int T, pad;
};
static_assert(sizeof(MatchProb) == 48, "descriptor layout is part of the ABI");
struct MatchProbs { MatchProb p[MC_MAX_PROB]; };

struct LsapProb {
    const float* cost;            // (Q, ld)
    long long* row_ind;           // min(Q, T) entries
    long long* col_ind;
    int T, ld;
};
static_assert(sizeof(LsapProb) == 32, "descriptor layout is part of the ABI");
struct LsapProbs { LsapProb p[LSAP_MAX_PROB]; };

static inline int mc_splits(int P) { const int nt = (P + MC_PT - 1) / MC_PT; return nt < MC_MAX_SPLIT ? nt : MC_MAX_SPLIT; }
__host__ __device__ static inline int mc_pad(int n) { return (n + MC_TILE - 1) / MC_TILE * MC_TILE; }
// floats per (problem, split): x.t and sigmoid(x).t as [Qp][Tp], then the two row sums [Qp] and the column sum [Tp]
__host__ __device__ static inline long mc_block_floats(int Qp, int Tp) { return 2L * Qp * Tp + 2L * Qp + Tp; }

// F.grid_sample(map, 2 * p - 1, mode="bilinear", padding_mode="zeros", align_corners=False) at one point: the four taps and weights in
// torch's arithmetic (unnormalise ((c + 1) * size - 1) / 2, weights from the corner differences), out-of-range taps dropped.
struct Taps { int x0, y0; float wnw, wne, wsw, wse; };
__device__ __forceinline__ Taps make_taps(float px, float py, int H, int W) {
    const float ix = ((2.f * px - 1.f + 1.f) * (float)W - 1.f) * 0.5f, iy = ((2.f * py - 1.f + 1.f) * (float)H - 1.f) * 0.5f;
    const float fx = floorf(ix), fy = floorf(iy);
    Taps t;
    // a coordinate far outside the map (or NaN) has no tap in range: park it where every bounds test fails
    t.x0 = (fx >= -2.f && fx <= (float)W) ? (int)fx : -4;
    t.y0 = (fy >= -2.f && fy <= (float)H) ? (int)fy : -4;
    const float ex = fx + 1.f - ix, ey = fy + 1.f - iy, dx = ix - fx, dy = iy - fy;
    t.wnw = ex * ey; t.wne = dx * ey; t.wsw = ex * dy; t.wse = dx * dy;
    return t;
}
template <typename T>
__device__ __forceinline__ float sample(const T* __restrict__ map, const Taps& t, int H, int W) {
    const bool xl = t.x0 >= 0 && t.x0 < W, xr = t.x0 + 1 >= 0 && t.x0 + 1 < W;
    const bool yt = t.y0 >= 0 && t.y0 < H, yb = t.y0 + 1 >= 0 && t.y0 + 1 < H;
    const long o = (long)t.y0 * W + t.x0;
    float v = 0.f;
    if (yt && xl) v += (float)map[o] * t.wnw;
    if (yt && xr) v += (float)map[o + 1] * t.wne;
    if (yb && xl) v += (float)map[o + W] * t.wsw;
    if (yb && xr) v += (float)map[o + W + 1] * t.wse;
    return v;
}

__global__ __launch_bounds__(256) void match_cost_partial_kernel(MatchProbs probs, int prob0, int Q, int h, int w, int Hg, int Wg, int P, int Tmax,
                                                                 int S, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) float xs[MC_PT][MC_TILE];     // x[k][q]
    __shared__ __attribute__((aligned(16))) float sg[MC_PT][MC_TILE];     // sigmoid(x)[k][q]
    __shared__ __attribute__((aligned(16))) float ts[MC_PT][MC_TILE];     // t[k][target]
    __shared__ float2 pts[MC_PT];
    const MatchProb pr = probs.p[blockIdx.z];
    const int Qp = mc_pad(Q), Tp = mc_pad(Tmax), ttiles = Tp / MC_TILE;
    const int qt = blockIdx.y / ttiles, tt = blockIdx.y % ttiles, split = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
    const int T = pr.T;
    float* out = ws + ((long)(prob0 + blockIdx.z) * S + split) * mc_block_floats(Qp, Tp);
    const int q0 = qt * MC_TILE, t0 = tt * MC_TILE;
    const bool work = q0 < Q && t0 < T;                   // a tile without queries or targets only writes zeros

    // sampling role: item `lane` (a query, then a target) at points grp, grp + 4, ...; contraction role: 4 x 4 outputs
    const int qs = q0 + lane, tg = t0 + lane;
    const float* xmap = pr.masks + (long)(qs < Q ? qs : 0) * h * w;
    const unsigned char* tmap = pr.gt + (long)(tg < T ? tg : 0) * Hg * Wg;
    const int cq = (tid >> 4) * 4, ct = (tid & 15) * 4;
    float ax[4][4], as[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) ax[a][b] = as[a][b] = 0.f;
    float r_sp = 0.f, r_sg = 0.f, c_t = 0.f;

    const int ntiles = (P + MC_PT - 1) / MC_PT;
    for (int tile = split; work && tile < ntiles; tile += S) {
        const int k0 = tile * MC_PT;
        __syncthreads();                                  // the previous tile's contraction has read xs / sg / ts
        if (tid < MC_PT) {
            const int k = k0 + tid;
            pts[tid] = k < P ? make_float2(pr.points[2L * k], pr.points[2L * k + 1]) : make_float2(0.f, 0.f);
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = grp; kk < MC_PT; kk += 4) {
            const bool live = k0 + kk < P;
            const float2 p = pts[kk];
            float x = 0.f, s = 0.f, t = 0.f;
            if (live && qs < Q) {
                x = sample(xmap, make_taps(p.x, p.y, h, w), h, w);
                const float e = expf(-fabsf(x)), d = 1.f / (1.f + e);
                s = x >= 0.f ? d : e * d;                 // sigmoid(x); NaN stays NaN
                r_sp += fmaxf(x, 0.f) + log1pf(e);        // softplus(x); a NaN comes through e
                r_sg += s;
            }
            if (live && tg < T) {
                t = sample(tmap, make_taps(p.x, p.y, Hg, Wg), Hg, Wg);
                c_t += t;
            }
            xs[kk][lane] = x; sg[kk][lane] = s; ts[kk][lane] = t;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < MC_PT; ++k) {
            const f32x4 xv = *(const f32x4*)&xs[k][cq], sv = *(const f32x4*)&sg[k][cq], tv = *(const f32x4*)&ts[k][ct];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    ax[a][b] = fmaf(xv[a], tv[b], ax[a][b]);
                    as[a][b] = fmaf(sv[a], tv[b], as[a][b]);
                }
        }
    }

    float* Ax = out, * As = out + (long)Qp * Tp;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long o = (long)(q0 + cq + a) * Tp + t0 + ct;
        *(f32x4*)(Ax + o) = f32x4{ax[a][0], ax[a][1], ax[a][2], ax[a][3]};
        *(f32x4*)(As + o) = f32x4{as[a][0], as[a][1], as[a][2], as[a][3]};
    }
    // row sums (from the workgroups of target tile 0) and column sums (query tile 0): the four point groups in a fixed order
    __syncthreads();
    float (*red)[4][MC_TILE] = (float (*)[4][MC_TILE])&xs[0][0];          // [3][4][64] floats, inside xs
    red[0][grp][lane] = r_sp; red[1][grp][lane] = r_sg; red[2][grp][lane] = c_t;
    __syncthreads();
    if (grp == 0) {
        float* Rsp = out + 2L * Qp * Tp, * Rsg = Rsp + Qp, * Ct = Rsg + Qp;
        if (tt == 0) {
            Rsp[q0 + lane] = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
            Rsg[q0 + lane] = ((red[1][0][lane] + red[1][1][lane]) + red[1][2][lane]) + red[1][3][lane];
        }
        if (qt == 0) Ct[t0 + lane] = ((red[2][0][lane] + red[2][1][lane]) + red[2][2][lane]) + red[2][3][lane];
    }
}

__global__ __launch_bounds__(64) void match_cost_finish_kernel(MatchProbs probs, int prob0, int Q, int C1, int P, int Tmax, int S, float w_class,
                                                               float w_mask, float w_dice, float nan_fill, const float* __restrict__ ws, float* __restrict__ cost) {
    const MatchProb pr = probs.p[blockIdx.y];
    const int q = blockIdx.x, lane = threadIdx.x, T = pr.T;
    const int Qp = mc_pad(Q), Tp = mc_pad(Tmax);
    const long blk = mc_block_floats(Qp, Tp);
    const float* base = ws + (long)(prob0 + blockIdx.y) * S * blk;
    float* row = cost + ((long)(prob0 + blockIdx.y) * Q + q) * Tmax;
    // softmax of the class logits of row q: exp(l - max) / sum, as torch computes it
    const float* lg = pr.logits + (long)q * C1;
    float m = -__builtin_inff();
    for (int c = lane; c < C1; c += 64) m = fmaxf(m, lg[c]);
    m = wave_max(m);
    float se = 0.f;
    for (int c = lane; c < C1; c += 64) se += expf(lg[c] - m);
    se = wave_sum(se);
    bool bad = false;                                     // fmaxf drops NaN: a NaN logit makes the whole softmax row NaN in torch
    for (int c = lane; c < C1; c += 64) bad |= lg[c] != lg[c];
    bad = __any(bad);
    double dsp = 0.0, dsg = 0.0;
    for (int s = 0; s < S; ++s) {
        const float* R = base + s * blk + 2L * Qp * Tp;
        dsp += (double)R[q]; dsg += (double)R[Qp + q];
    }
    const float rsp = (float)dsp, rsg = (float)dsg;
    for (int t = lane; t < Tmax; t += 64) {
        float c = 0.f;
        if (t < T) {
            double dxt = 0.0, dst = 0.0, dct = 0.0;
            for (int s = 0; s < S; ++s) {
                const float* B = base + s * blk;
                dxt += (double)B[(long)q * Tp + t];
                dst += (double)B[(long)Qp * Tp + (long)q * Tp + t];
                dct += (double)B[2L * Qp * Tp + 2L * Qp + t];
            }
            const float cost_mask = (rsp - (float)dxt) / (float)P;
            const float cost_dice = 1.f - (2.f * (float)dst + 1.f) / (rsg + (float)dct + 1.f);
            const long long lab = pr.labels[t];
            const float cost_class = (bad || lab < 0 || lab >= C1) ? __builtin_nanf("") : -(expf(lg[lab] - m) / se);
            c = (w_mask * cost_mask + w_class * cost_class) + w_dice * cost_dice;
            if (c != c) c = nan_fill;                      // 100: matcher.py:33-34
        }
        row[t] = c;                                       // columns >= T are written as zero
    }
}

extern "C" long uenc_match_cost_workspace_floats(int n_prob, int Q, int Tmax, int P) {
    if (n_prob < 1 || Q < 1 || Q > LSAP_MAX_N || Tmax < 1 || Tmax > LSAP_MAX_N || P < 1) return -1;
    return (long)n_prob * mc_splits(P) * mc_block_floats(mc_pad(Q), mc_pad(Tmax));
}

extern "C" int uenc_match_cost(const void* probs, int n_prob, int Q, int C1, int h, int w, int Hg, int Wg, int P, int Tmax, float w_class,
                               float w_mask, float w_dice, float nan_fill, float* workspace, long workspace_floats, float* cost, hipStream_t stream) {
    UENC_CHECK_ARG(probs != nullptr && workspace != nullptr && cost != nullptr && n_prob >= 1 && n_prob <= 4096);
    UENC_CHECK_ARG(Q >= 1 && Q <= LSAP_MAX_N && Tmax >= 1 && Tmax <= LSAP_MAX_N && C1 >= 1 && C1 <= 65536);
    UENC_CHECK_ARG(h >= 1 && w >= 1 && Hg >= 1 && Wg >= 1 && h <= 16384 && w <= 16384 && Hg <= 16384 && Wg <= 16384 && P >= 1 && P <= (1 << 24));
    UENC_CHECK_ARG((((uintptr_t)workspace) & 15) == 0 && (((uintptr_t)cost) & 3) == 0);
    UENC_CHECK_ARG(workspace_floats >= uenc_match_cost_workspace_floats(n_prob, Q, Tmax, P));
    const MatchProb* hp = (const MatchProb*)probs;
    for (int i = 0; i < n_prob; ++i) {
        UENC_CHECK_ARG(hp[i].T >= 0 && hp[i].T <= Tmax && hp[i].logits != nullptr && hp[i].masks != nullptr && hp[i].points != nullptr);
        UENC_CHECK_ARG(hp[i].T == 0 || (hp[i].gt != nullptr && hp[i].labels != nullptr));
        UENC_CHECK_ARG((((uintptr_t)hp[i].logits | (uintptr_t)hp[i].masks | (uintptr_t)hp[i].points) & 3) == 0 && (((uintptr_t)hp[i].labels) & 7) == 0);
    }
    const int S = mc_splits(P), tiles = (mc_pad(Q) / MC_TILE) * (mc_pad(Tmax) / MC_TILE);
    for (int p0 = 0; p0 < n_prob; p0 += MC_MAX_PROB) {
        const int n = n_prob - p0 < MC_MAX_PROB ? n_prob - p0 : MC_MAX_PROB;
        MatchProbs args;
        for (int i = 0; i < MC_MAX_PROB; ++i) args.p[i] = hp[p0 + (i < n ? i : 0)];
        hipLaunchKernelGGL(match_cost_partial_kernel, dim3(S, tiles, n), dim3(256), 0, stream, args, p0, Q, h, w, Hg, Wg, P, Tmax, S, workspace);
        hipLaunchKernelGGL(match_cost_finish_kernel, dim3(Q, n), dim3(64), 0, stream, args, p0, Q, C1, P, Tmax, S, w_class, w_mask, w_dice,
                           nan_fill, (const float*)workspace, cost);
    }
    UENC_LAUNCH_RET();
}

// ---- linear sum assignment ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lsap_clean(float c) { return c != c ? 100.f : fminf(fmaxf(c, -1e30f), 1e30f); }

__global__ __launch_bounds__(256) void lsap_kernel(LsapProbs probs, int Q) {
    __shared__ float cs[LSAP_LDS_ENTRIES];
    __shared__ double u[LSAP_MAX_N];
    __shared__ int col4row[LSAP_MAX_N], row4col[LSAP_MAX_N], path[LSAP_MAX_N];
    __shared__ double red_v[2][4];
    __shared__ int red_k[2][4];
    __shared__ int wave_cnt[4];
    const LsapProb pr = probs.p[blockIdx.x];
    const int T = pr.T, ld = pr.ld;
    if (T <= 0) return;
    // scipy solves the transposed problem when there are more rows than columns: rows = the smaller side
    const bool tr = T < Q;
    const int nr = tr ? T : Q, nc = tr ? Q : T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = tid;
    const bool mine = j < nc;
    const bool in_lds = nr * nc <= LSAP_LDS_ENTRIES;
    const float* __restrict__ C = pr.cost;
    if (in_lds)
        for (int e = tid; e < Q * T; e += 256) {
            const int q = e / T, t = e - q * T;
            cs[tr ? t * nc + q : q * nc + t] = lsap_clean(C[(long)q * ld + t]);
        }
    u[tid] = 0.0; col4row[tid] = -1; row4col[tid] = -1; path[tid] = -1;
    __syncthreads();

    double v = 0.0;
    int r4c = -1, parity = 0;
    bool failed = false;
    for (int cur = 0; cur < nr && !failed; ++cur) {
        double sp = 1.7e308, minVal = 0.0;
        bool visited = false;
        int pth = -1, i = cur, sink = -1;
        for (int step = 0; step <= nc && sink < 0; ++step) {
            double key = 1.79e308;
            int kk = 1023;
            if (mine && !visited) {
                const float c = in_lds ? cs[i * nc + j] : lsap_clean(tr ? C[(long)j * ld + i] : C[(long)i * ld + j]);
                const double r = minVal + (double)c - u[i] - v;
                if (r < sp) { sp = r; pth = i; }
                key = sp;
                kk = (r4c < 0 ? 0 : 256) + j;             // among equal path costs an unassigned column (a sink) first, as scipy does
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ok = __shfl_xor(key, o);
                const int okk = __shfl_xor(kk, o);
                if (ok < key || (ok == key && okk < kk)) { key = ok; kk = okk; }
            }
            if (lane == 0) { red_v[parity][wave] = key; red_k[parity][wave] = kk; }
            __syncthreads();
            key = red_v[parity][0]; kk = red_k[parity][0];
#pragma unroll
            for (int wv = 1; wv < 4; ++wv) {
                const double ok = red_v[parity][wv];
                const int okk = red_k[parity][wv];
                if (ok < key || (ok == key && okk < kk)) { key = ok; kk = okk; }
            }
            parity ^= 1;
            if (kk == 1023) { failed = true; break; }     // no column left: cannot happen with finite costs (nr <= nc)
            minVal = key;
            const int jm = kk & 255;
            if (j == jm) visited = true;
            const int rj = row4col[jm];
            if (rj < 0) sink = jm; else i = rj;
        }
        if (sink < 0) { failed = true; break; }
        // dual update (before the augmentation re-points row4col), then the augmentation along `path` by one lane
        if (tid == 0) u[cur] += minVal;
        if (mine && visited) {
            if (j != sink) u[r4c] += minVal - sp;
            v -= minVal - sp;
        }
        path[j] = pth;
        __syncthreads();
        if (tid == 0) {
            int jj = sink;
            for (int n = 0; n <= nr; ++n) {
                const int ii = path[jj];
                row4col[jj] = ii;
                const int prev = col4row[ii];
                col4row[ii] = jj;
                jj = prev;
                if (ii == cur) break;
            }
        }
        __syncthreads();
        r4c = row4col[j];
    }

    if (failed) {
        if (tid < nr) { pr.row_ind[tid] = -1; pr.col_ind[tid] = -1; }
        return;
    }
    if (!tr) {                                            // rows are the queries: all of them matched, in order
        if (tid < nr) { pr.row_ind[tid] = tid; pr.col_ind[tid] = col4row[tid]; }
        return;
    }
    // columns are the queries: the matched ones in ascending order (scipy sorts the transposed solution by row)
    const bool has = mine && r4c >= 0;
    const unsigned long long bal = __ballot(has);
    if (lane == 0) wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    int pos = __popcll(bal & ((1ull << lane) - 1ull));
    for (int wv = 0; wv < wave; ++wv) pos += wave_cnt[wv];
    if (has) { pr.row_ind[pos] = j; pr.col_ind[pos] = r4c; }
}

extern "C" int uenc_lsap_solve(const void* probs, int n_prob, int Q, hipStream_t stream) {
    UENC_CHECK_ARG(probs != nullptr && n_prob >= 1 && n_prob <= 65536 && Q >= 1 && Q <= LSAP_MAX_N);
    const LsapProb* hp = (const LsapProb*)probs;
    for (int i = 0; i < n_prob; ++i) {
        UENC_CHECK_ARG(hp[i].T >= 0 && hp[i].T <= LSAP_MAX_N && hp[i].ld >= hp[i].T);
        UENC_CHECK_ARG(hp[i].T == 0 || (hp[i].cost != nullptr && hp[i].row_ind != nullptr && hp[i].col_ind != nullptr));
        UENC_CHECK_ARG((((uintptr_t)hp[i].cost) & 3) == 0 && (((uintptr_t)hp[i].row_ind | (uintptr_t)hp[i].col_ind) & 7) == 0);
    }
    for (int p0 = 0; p0 < n_prob; p0 += LSAP_MAX_PROB) {
        const int n = n_prob - p0 < LSAP_MAX_PROB ? n_prob - p0 : LSAP_MAX_PROB;
        LsapProbs args;
        for (int i = 0; i < LSAP_MAX_PROB; ++i) args.p[i] = hp[p0 + (i < n ? i : 0)];
        hipLaunchKernelGGL(lsap_kernel, dim3(n), dim3(256), 0, stream, args, Q);
    }
    UENC_LAUNCH_RET();
}
