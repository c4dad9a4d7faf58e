// The per-image segment-id -> table-row lookup shared by the kernels that walk a panoptic id map (targets.hip, evalstats.hip): the chunk
// geometry of their (chunks, B) grids and one LDS table per workgroup: 512 cells of open addressing for at most 256 ids (load <= 1 / 2),
// exact for any id: a probe ends at the id or at an empty cell, and an id that is in the map but not in the table finds an empty one.
#pragma once
#include "common.h"

#define TG_THREADS 256
#define TG_PIX 16                          // pixels per thread and chunk
#define TG_CHUNK (TG_THREADS * TG_PIX)
#define TG_ROWS 256                        // table rows per image: UENC_TARGETS_MAX_SEGMENTS
#define TG_CELLS 512
#define TG_MAX_BLOCKS 512                  // workgroups per image; further chunks are taken in a grid-stride loop

struct TgTable {
    int key[TG_CELLS];                     // 0 = empty (ids are > 0)
    int row[TG_CELLS];
};

__device__ __forceinline__ unsigned tg_hash(int id) { return ((unsigned)id * 2654435761u) >> 23; }      // 9 bits

// n ids of one image into the table; an id <= 0 gets no cell, of two equal ids the lower row wins.  Ends with a barrier.
__device__ __forceinline__ void tg_build(TgTable& tb, const int* __restrict__ ids, int n) {
    for (int i = threadIdx.x; i < TG_CELLS; i += TG_THREADS) {
        tb.key[i] = 0;
        tb.row[i] = 0x7fffffff;
    }
    __syncthreads();
    for (int r = threadIdx.x; r < n; r += TG_THREADS) {
        const int id = ids[r];
        if (id <= 0) continue;
        unsigned c = tg_hash(id);
        for (int probe = 0; probe < TG_CELLS; ++probe) {
            const int old = atomicCAS(&tb.key[c], 0, id);
            if (old == 0 || old == id) {
                atomicMin(&tb.row[c], r);
                break;
            }
            c = (c + 1) & (TG_CELLS - 1);
        }
    }
    __syncthreads();
}

__device__ __forceinline__ int tg_lookup(const TgTable& tb, int id) {
    if (id <= 0) return -1;
    unsigned c = tg_hash(id);
    for (int probe = 0; probe < TG_CELLS; ++probe) {
        const int k = tb.key[c];
        if (k == id) return tb.row[c];
        if (k == 0) return -1;
        c = (c + 1) & (TG_CELLS - 1);
    }
    return -1;
}

// The row of a pixel's id, through the thread's memory of the last id it looked up.
struct TgLast {
    int id = 0, row = -1;
    __device__ __forceinline__ int operator()(const TgTable& tb, int v) {
        if (v != id) {
            id = v;
            row = tg_lookup(tb, v);
        }
        return row;
    }
};

__device__ __forceinline__ int tg_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static inline bool tg_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static inline int tg_blocks(int H, int W) {
    const int chunks = (int)ceil_div64((int64_t)H * W, TG_CHUNK);
    return chunks < TG_MAX_BLOCKS ? chunks : TG_MAX_BLOCKS;
}
