// Shared between na2d.hip (launch entry points; VALU kernels: window sizes >= 9, and <= 7 on maps past the MFMA kernels' 32-bit
// index range) and na2d_mfma.hip (MFMA kernels: window sizes <= 7 -- na2d_mfma_supported is the routing predicate).
#pragma once
#include "common.h"

struct Na2d {
    const bf16* qkv; const float* rpb; bf16* out; float* lse;
    const bf16* dout; bf16* dqkv; float* drpb; float* delta;
    int B, H, W, nH, d;
    float scale;
    int hh_max, hw_max;      // MFMA bwd_kv: LDS halo extents (class positions) for this launch
    int tiles_x, tiles_y, nt; float inv_tiles_x;     // MFMA kernels: tiles per residue class, tiles per workgroup
};

struct AxisWin { int start, r, pb0; };       // first class position of the window, residue, bias index of slot 0

__device__ __forceinline__ AxisWin axis_win(int t, int len, int d, int K) {
    AxisWin a;
    a.r = t % d;
    const int p = t / d, L = (len - a.r + d - 1) / d;
    a.start = min(max(p - K / 2, 0), L - K);
    a.pb0 = a.start - p + K - 1;
    return a;
}

static int na2d_check(const Na2d& p, int K) {
    UENC_CHECK_ARG(p.B > 0 && p.H > 0 && p.W > 0 && p.nH > 0 && p.d >= 1);
    UENC_CHECK_ARG(K >= 3 && K <= 13 && (K & 1));
    UENC_CHECK_ARG(p.H >= K * p.d && p.W >= K * p.d);      // the caller zero-pads smaller inputs first, like NATTEN
    UENC_CHECK_ARG((long)p.B * p.nH <= 65535 && p.H <= 65535);
    return UENC_OK;
}

// na2d_mfma.hip
int na2d_mfma_fwd(const Na2d& p, int K, hipStream_t stream);
int na2d_mfma_bwd(Na2d& p, int K, hipStream_t stream);
bool na2d_mfma_supported(int H, int W, int nH, int K);
// the MFMA kernels' schedule: tiles per residue class, consecutive tiles per workgroup (nt), workgroups per class (chunks)
struct NmPlan { int tiles_x, tiles_y, nt, chunks; };
NmPlan na2d_mfma_plan(int B, int H, int W, int nH, int d);
