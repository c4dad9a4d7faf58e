// Training targets from a panoptic id map, built on the device (uenc/modeling/targets.py; the rules are the reference's
// model/data/dataset_mappers/oneformer_unified_dataset_mapper.py:138-283, which builds one boolean mask per segment with numpy on the
// host: 236 ms and 84 MB of masks to upload per 1024 x 2048 image with 40 segments).
//
//   uenc_targets_area   area[b, r] = number of pixels of image b, inside its own (h_b, w_b), whose id is seg_ids[b, r]
//   uenc_targets_write  masks[plane0[b] + t, y, x] = 1 where slot[b, row(y, x)] == t, else 0;  sem_seg[b, y, x] = cls[b, row(y, x)], or
//                       ignore_label where the pixel has no row, the row's cls is < 0, or the pixel is padding
//
// Both run over one padded batch pan (B, H, W) int32 with grid (chunks, B): a workgroup serves chunks of 4096 pixels of ONE image,
// so that the image's id -> row lookup is one LDS table per workgroup: 512 cells of open addressing for at most 256 ids (load <= 1 / 2),
// exact for any id: a probe ends at the id or at an empty cell, and an id that is in the map but not in the table finds an empty one.
// Segment maps are piecewise constant, so a thread remembers its last (id, row) and probes only where the id changes.
//
// Bound: HBM stores.  The write kernel reads the map once (4 B per pixel, 16-byte loads) and stores T_b + 8 bytes per pixel, every
// byte once, 16 bytes per lane and plane: consecutive lanes fill consecutive 16-byte pieces, 1 KiB per wave store.  The area kernel
// counts in LDS (run lengths of equal rows first) and adds one integer per (workgroup, row) to global memory: integer sums do not
// depend on the order.  When H * W is no multiple of 16 (or a base pointer is not 16-byte aligned) the planes of one batch are not all
// 16-byte aligned: a lane then takes one pixel at a time and consecutive lanes consecutive pixels.
#include "common.h"

#include "tg_table.h"                      // the id -> row table and the chunk geometry, shared with evalstats.hip

// ---- area ----------------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(TG_THREADS) void targets_area_kernel(const int* __restrict__ pan, const int* __restrict__ sizes,
                                                                  const int* __restrict__ seg_ids, const int* __restrict__ n_seg,
                                                                  int* __restrict__ area, int H, int W) {
    __shared__ TgTable tb;
    __shared__ int cnt[TG_ROWS];
    const int b = blockIdx.y;
    const int n = tg_clamp(n_seg[b], 0, TG_ROWS);
    const int h = tg_clamp(sizes[2 * b], 0, H), w = tg_clamp(sizes[2 * b + 1], 0, W);
    cnt[threadIdx.x] = 0;
    tg_build(tb, seg_ids + (size_t)b * TG_ROWS, n);

    const int HW = H * W;
    const int* __restrict__ img = pan + (size_t)b * HW;
    const int chunks = (HW + TG_CHUNK - 1) / TG_CHUNK;
    TgLast last;
    int run_row = -1, run = 0;
    auto count = [&](int row) {
        if (row != run_row) {
            if (run_row >= 0) atomicAdd(&cnt[run_row], run);
            run_row = row;
            run = 0;
        }
        ++run;
    };
    for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
        if (VEC) {
            const int p0 = c * TG_CHUNK + threadIdx.x * TG_PIX;
            if (p0 >= HW) continue;                                        // HW % 16 == 0: a thread's 16 pixels are all in or all out
            int y = p0 / W, x = p0 - y * W;
#pragma unroll
            for (int q = 0; q < TG_PIX / 4; ++q) {
                const int4 v = *reinterpret_cast<const int4*>(img + p0 + 4 * q);
                const int id[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    count((y < h && x < w) ? last(tb, id[i]) : -1);
                    if (++x == W) { x = 0; ++y; }
                }
            }
        } else {
#pragma unroll 4
            for (int i = 0; i < TG_PIX; ++i) {
                const int p = c * TG_CHUNK + i * TG_THREADS + threadIdx.x;
                if (p >= HW) break;
                const int y = p / W, x = p - y * W;
                count((y < h && x < w) ? last(tb, img[p]) : -1);
            }
        }
    }
    if (run_row >= 0) atomicAdd(&cnt[run_row], run);
    __syncthreads();
    const int mine = cnt[threadIdx.x];
    if (threadIdx.x < n && mine) atomicAdd(&area[(size_t)b * TG_ROWS + threadIdx.x], mine);
}

// ---- write ---------------------------------------------------------------------------------------------------------------------------------
// 0x01 in every byte of x that equals the byte t of every lane of tt, where the same byte of valid is 0x01
__device__ __forceinline__ unsigned tg_eq_bytes(unsigned x, unsigned tt, unsigned valid) {
    const unsigned d = x ^ tt;                                                         // a byte is 0 where it equals t
    const unsigned nz = (((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u;          // 0x80 where the byte is not 0: no carry leaves a byte
    return ((nz ^ 0x80808080u) >> 7) & valid;
}

template <bool VEC>
__global__ __launch_bounds__(TG_THREADS) void targets_write_kernel(const int* __restrict__ pan, const int* __restrict__ sizes,
                                                                   const int* __restrict__ seg_ids, const int* __restrict__ n_seg,
                                                                   const int* __restrict__ slot, const int* __restrict__ cls,
                                                                   const int* __restrict__ plane0, const int* __restrict__ Tn,
                                                                   long long ignore_label, unsigned char* __restrict__ masks,
                                                                   long long* __restrict__ sem_seg, int H, int W, int total_planes) {
    __shared__ TgTable tb;
    __shared__ int s_slot[TG_ROWS], s_cls[TG_ROWS];
    const int b = blockIdx.y;
    const int n = tg_clamp(n_seg[b], 0, TG_ROWS);
    const int h = tg_clamp(sizes[2 * b], 0, H), w = tg_clamp(sizes[2 * b + 1], 0, W);
    // the planes of this image: nothing is stored outside [0, total_planes)
    int T = tg_clamp(Tn[b], 0, TG_ROWS);
    const int pl0 = plane0[b];
    if (pl0 < 0 || pl0 > total_planes - T) T = 0;
    {
        const int r = threadIdx.x;
        const int s = r < n ? slot[(size_t)b * TG_ROWS + r] : -1;
        s_slot[r] = (s >= 0 && s < T) ? s : -1;
        s_cls[r] = r < n ? cls[(size_t)b * TG_ROWS + r] : -1;
    }
    tg_build(tb, seg_ids + (size_t)b * TG_ROWS, n);

    const int HW = H * W;
    const int* __restrict__ img = pan + (size_t)b * HW;
    long long* __restrict__ sem = sem_seg + (size_t)b * HW;
    unsigned char* __restrict__ planes = masks + (size_t)pl0 * HW;          // dereferenced for t < T only
    const int chunks = (HW + TG_CHUNK - 1) / TG_CHUNK;
    TgLast last;
    for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
        if (VEC) {
            const int p0 = c * TG_CHUNK + threadIdx.x * TG_PIX;
            if (p0 >= HW) continue;
            int y = p0 / W, x = p0 - y * W;
            unsigned sl[TG_PIX / 4], ok[TG_PIX / 4];                        // four pixels' slot bytes / 0x01 where the pixel has a slot
#pragma unroll
            for (int q = 0; q < TG_PIX / 4; ++q) {
                const int4 v = *reinterpret_cast<const int4*>(img + p0 + 4 * q);
                const int id[4] = {v.x, v.y, v.z, v.w};
                long long lab[4];
                sl[q] = ok[q] = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = (y < h && x < w) ? last(tb, id[i]) : -1;
                    const int s = row >= 0 ? s_slot[row] : -1;
                    const int k = row >= 0 ? s_cls[row] : -1;
                    lab[i] = k >= 0 ? (long long)k : ignore_label;
                    if (s >= 0) {
                        sl[q] |= (unsigned)s << (8 * i);
                        ok[q] |= 1u << (8 * i);
                    }
                    if (++x == W) { x = 0; ++y; }
                }
                longlong2* out = reinterpret_cast<longlong2*>(sem + p0 + 4 * q);
                out[0] = make_longlong2(lab[0], lab[1]);
                out[1] = make_longlong2(lab[2], lab[3]);
            }
            for (int t = 0; t < T; ++t) {
                const unsigned tt = (unsigned)t * 0x01010101u;
                u32x4 o;
#pragma unroll
                for (int q = 0; q < TG_PIX / 4; ++q) o[q] = tg_eq_bytes(sl[q], tt, ok[q]);
                *reinterpret_cast<u32x4*>(planes + (size_t)t * HW + p0) = o;
            }
        } else {
            for (int i = 0; i < TG_PIX; ++i) {
                const int p = c * TG_CHUNK + i * TG_THREADS + threadIdx.x;
                if (p >= HW) break;
                const int y = p / W, x = p - y * W;
                const int row = (y < h && x < w) ? last(tb, img[p]) : -1;
                const int s = row >= 0 ? s_slot[row] : -1;
                const int k = row >= 0 ? s_cls[row] : -1;
                sem[p] = k >= 0 ? (long long)k : ignore_label;
                for (int t = 0; t < T; ++t) planes[(size_t)t * HW + p] = (unsigned char)(s == t);
            }
        }
    }
}

extern "C" int uenc_targets_area(const int* pan, const int* sizes, const int* seg_ids, const int* n_seg, int* area, int B, int H, int W,
                                 hipStream_t stream) {
    UENC_CHECK_ARG(pan && sizes && seg_ids && n_seg && area);
    UENC_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= 0x7fffffff - TG_CHUNK);
    const dim3 grid(tg_blocks(H, W), B), block(TG_THREADS);
    if (((int64_t)H * W) % TG_PIX == 0 && tg_aligned16(pan))
        hipLaunchKernelGGL(targets_area_kernel<true>, grid, block, 0, stream, pan, sizes, seg_ids, n_seg, area, H, W);
    else
        hipLaunchKernelGGL(targets_area_kernel<false>, grid, block, 0, stream, pan, sizes, seg_ids, n_seg, area, H, W);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_targets_write(const int* pan, const int* sizes, const int* seg_ids, const int* n_seg, const int* slot, const int* cls,
                                  const int* plane0, const int* T, long long ignore_label, unsigned char* masks, long long* sem_seg, int B,
                                  int H, int W, int total_planes, hipStream_t stream) {
    UENC_CHECK_ARG(pan && sizes && seg_ids && n_seg && slot && cls && plane0 && T && sem_seg);
    UENC_CHECK_ARG(total_planes >= 0 && (masks || total_planes == 0));
    UENC_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= 0x7fffffff - TG_CHUNK);
    const dim3 grid(tg_blocks(H, W), B), block(TG_THREADS);
    if (((int64_t)H * W) % TG_PIX == 0 && tg_aligned16(pan) && tg_aligned16(masks) && tg_aligned16(sem_seg))
        hipLaunchKernelGGL(targets_write_kernel<true>, grid, block, 0, stream, pan, sizes, seg_ids, n_seg, slot, cls, plane0, T, ignore_label, masks,
                           sem_seg, H, W, total_planes);
    else
        hipLaunchKernelGGL(targets_write_kernel<false>, grid, block, 0, stream, pan, sizes, seg_ids, n_seg, slot, cls, plane0, T, ignore_label,
                           masks, sem_seg, H, W, total_planes);
    UENC_LAUNCH_RET();
}
