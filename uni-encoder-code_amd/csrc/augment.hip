// Training-time augmentation of one sample on the device (uenc/train_data.py: apply_plans).  The reference resizes every full frame with
// PIL on the host, then crops most of it away and runs the SSD colour augmentation over what is left; the plan (resized size, crop window,
// flip, pad, colour parameters) is known before any pixel is touched, so these kernels compute the window only.
//
//   uenc_augment_image   F source frames (HWC uint8) -> (F, 3, out_h, out_w) uint8 planes: PIL's antialiased BILINEAR resize restricted to
//                        the crop window (a horizontal pass into a uint8 intermediate, then a vertical pass, 22-bit fixed-point
//                        coefficients from the host), the SSD colour stages (value tables from the host, OpenCV-style 8-bit HSV),
//                        horizontal flip, pad / crop to the output size
//   uenc_augment_labels  the panoptic PNG (HWC uint8) -> int32 id map and the label map -> int32, gathered through the host's nearest
//                        row / column index tables over the same window, flip and pad
//
// Image kernel: one workgroup of 256 threads makes one 64 x 16 tile of ONE frame's output.  The tile's taps span <= AUG_ROWS source rows
// and <= AUG_PIX source pixels per row (checked on the host from the scale factors, clamped again here).  Stages, each ended by a barrier:
//   1. wave 0 loads the tile's 64 column records (first tap, tap count, coefficients), wave 1 its 16 row records, waves 2-3 the colour
//      tables; the source rectangle is the min / max over the records (wave reductions);
//   2. the rectangle's rows are copied to LDS with 16-byte loads from 16-byte aligned addresses: HWC rows of 3-byte pixels start at
//      any byte, so every row keeps its own shift (address & 15); a chunk that would reach outside the frame is read byte by byte;
//   3. horizontal pass: (row, column) -> three channels of the uint8 intermediate, PIL's rounding ((1 << 21) + sum) >> 22, clipped;
//   4. vertical pass from the intermediate, colour in registers, and the store: a thread owns four consecutive output pixels of one row
//      and writes one 32-bit word per plane (bytes at a ragged edge).  The flip is applied where the column records are loaded (column j
//      of the tile reads window column cw - 1 - x), so the stores stay in address order.
// LDS: 40 x 512 (source) + 40 x 192 (intermediate) + 2.9 KB (records) + 2.8 KB (colour) = 33.8 KB -> four workgroups per CU.
// Bound: the kernel reads every source byte of the window about (1 + halo) times and writes 3 bytes per output pixel; the taps are integer
// multiply-adds from LDS.  No atomics, nothing is read back, no allocation.
//
// The float stage (HSV -> BGR) must give the bits of the host's float32 numpy expression: every operation below is a single rounded
// IEEE operation, and contraction into fused multiply-adds is switched off for this file.
#pragma clang fp contract(off)
#include "common.h"

#define AUG_TW UENC_AUG_TILE_W
#define AUG_TH UENC_AUG_TILE_H
#define AUG_THREADS 256
#define AUG_TAPS UENC_AUG_MAX_TAPS
#define AUG_ROWS 40                         // source rows of one tile
#define AUG_RAW 512                         // bytes of one staged source row, its shift included
#define AUG_PIX ((AUG_RAW - 16) / 3)        // 165 source pixels per row

static_assert(AUG_TW == 64 && AUG_TH * (AUG_TW / 4) == AUG_THREADS, "a thread owns four pixels of the tile");

enum { AUG_SAT = 1, AUG_HUE = 2, AUG_CONTRAST_FIRST = 4, AUG_RGB = 8 };     // UENC_AUG_COLOUR_*

__device__ __forceinline__ int aug_clip8(int acc) {
    const int v = acc >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// OpenCV's 8-bit BGR -> HSV (H in [0, 180)), integers only; sdiv / hdiv are the host's rounded reciprocal tables
__device__ __forceinline__ void aug_bgr2hsv(int b, int g, int r, const int* sdiv, const int* hdiv, int& h, int& s, int& v) {
    v = max(b, max(g, r));
    const int diff = v - min(b, min(g, r));
    s = (diff * sdiv[v] + (1 << 11)) >> 12;
    int hh;
    if (v == r) hh = g - b;
    else if (v == g) hh = b - r + 2 * diff;
    else hh = r - g + 4 * diff;
    hh = (hh * hdiv[diff] + (1 << 11)) >> 12;
    h = hh < 0 ? hh + 180 : hh;
}

__device__ __forceinline__ int aug_round8(float x) {
    const float y = x * 255.f;
    const int i = __float2int_rn(y);                                        // round half to even (cvRound)
    return i < 0 ? 0 : (i > 255 ? 255 : i);
}

// OpenCV's 8-bit HSV -> BGR: float32, one rounded operation per line of the host's expression
__device__ __forceinline__ void aug_hsv2bgr(int h, int s, int v, int& b, int& g, int& r) {
    const float sf = (float)s * (1.f / 255.f), vf = (float)v * (1.f / 255.f);
    if (s == 0) {
        b = g = r = aug_round8(vf);
        return;
    }
    float hf = (float)h * (6.f / 180.f);
    if (hf >= 6.f) hf = hf - 6.f;
    int sector = (int)floorf(hf);
    float f = hf - (float)sector;
    if ((unsigned)sector >= 6u) {
        sector = 0;
        f = 0.f;
    }
    const float t0 = vf;
    const float t1 = vf * (1.f - sf);
    const float t2 = vf * (1.f - sf * f);
    const float t3 = vf * (1.f - sf * (1.f - f));
    float fb, fg, fr;
    switch (sector) {
        case 0: fb = t1; fg = t3; fr = t0; break;
        case 1: fb = t1; fg = t0; fr = t2; break;
        case 2: fb = t3; fg = t0; fr = t1; break;
        case 3: fb = t0; fg = t2; fr = t1; break;
        case 4: fb = t0; fg = t1; fr = t3; break;
        default: fb = t2; fg = t1; fr = t0; break;
    }
    b = aug_round8(fb);
    g = aug_round8(fg);
    r = aug_round8(fr);
}

// The SSD colour stages on one pixel, in the image's own channel order c0 c1 c2 (RGB when AUG_RGB, else BGR)
__device__ __forceinline__ void aug_colour(int& c0, int& c1, int& c2, int flags, int hue, const unsigned char* lut, const int* sdiv,
                                           const int* hdiv) {
    int b = (flags & AUG_RGB) ? c2 : c0, g = c1, r = (flags & AUG_RGB) ? c0 : c2;
    b = lut[b]; g = lut[g]; r = lut[r];                                     // brightness (identity table when off)
    if (flags & AUG_CONTRAST_FIRST) { b = lut[256 + b]; g = lut[256 + g]; r = lut[256 + r]; }
    int h, s, v;
    if (flags & AUG_SAT) {
        aug_bgr2hsv(b, g, r, sdiv, hdiv, h, s, v);
        aug_hsv2bgr(h, lut[512 + s], v, b, g, r);
    }
    if (flags & AUG_HUE) {
        aug_bgr2hsv(b, g, r, sdiv, hdiv, h, s, v);
        h = ((h + hue) % 180 + 180) % 180;
        aug_hsv2bgr(h, s, v, b, g, r);
    }
    if (!(flags & AUG_CONTRAST_FIRST)) { b = lut[256 + b]; g = lut[256 + g]; r = lut[256 + r]; }
    c0 = (flags & AUG_RGB) ? r : b;
    c1 = g;
    c2 = (flags & AUG_RGB) ? b : r;
}

__device__ __forceinline__ int aug_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int aug_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(AUG_THREADS) void augment_image_kernel(const unsigned char* __restrict__ src, long frame_stride, int in_h, int in_w,
                                                                    const int* __restrict__ col_tab, int kx, const int* __restrict__ row_tab,
                                                                    int ky, int cw, int ch, const int* __restrict__ ctab, int cflags, int hue,
                                                                    int flip, int out_h, int out_w, int pad, unsigned char* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) unsigned char raw[AUG_ROWS][AUG_RAW];
    __shared__ unsigned char mid[AUG_ROWS][AUG_TW * 3];
    __shared__ int cxmin[AUG_TW], cn[AUG_TW], ck[AUG_TW * AUG_TAPS];
    __shared__ int rymin[AUG_TH], rn[AUG_TH], rk[AUG_TH * AUG_TAPS];
    __shared__ __attribute__((aligned(4))) unsigned char lut[768];
    __shared__ int sdiv[256], hdiv[256];
    __shared__ int rect[4];                                                 // sx0, pixels per row, sy0, rows
    __shared__ unsigned char shift[AUG_ROWS];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tx0 = blockIdx.x * AUG_TW, ty0 = blockIdx.y * AUG_TH, f = blockIdx.z;
    const int nx = min(max(min(cw, out_w) - tx0, 0), AUG_TW), ny = min(max(min(ch, out_h) - ty0, 0), AUG_TH);
    const unsigned char* __restrict__ frame = src + (size_t)f * frame_stride;
    const unsigned char* frame_end = frame + (size_t)in_h * in_w * 3;
    const bool inside = nx > 0 && ny > 0;                                   // else the tile is padding only

    // ---- 1. records and colour tables ----------------------------------------------------------------------------------------------
    if (inside) {
        if (wave == 0) {
            int x0 = 0x7fffffff, x1 = 0, n = 0;
            if (lane < nx) {
                const int wx = flip ? cw - 1 - (tx0 + lane) : tx0 + lane;
                x0 = min(max(col_tab[wx], 0), in_w);
                n = min(max(col_tab[cw + wx], 0), min(kx, in_w - x0));
                x1 = x0 + n;
                for (int i = 0; i < kx; ++i) ck[lane * AUG_TAPS + i] = col_tab[2 * cw + wx * kx + i];
            }
            const int lo = min(aug_wave_min(x0), in_w), hi = aug_wave_max(x1);
            const int npx = min(max(hi - lo, 0), AUG_PIX);
            if (lane < nx) {
                cxmin[lane] = x0 - lo;
                cn[lane] = max(min(n, npx - (x0 - lo)), 0);                  // a record that reaches past the staged pixels loses its tail
            }
            if (lane == 0) { rect[0] = lo; rect[1] = npx; }
        } else if (wave == 1) {
            int y0 = 0x7fffffff, y1 = 0, n = 0;
            if (lane < ny) {
                const int wy = ty0 + lane;
                y0 = min(max(row_tab[wy], 0), in_h);
                n = min(max(row_tab[ch + wy], 0), min(ky, in_h - y0));
                y1 = y0 + n;
                for (int i = 0; i < ky; ++i) rk[lane * AUG_TAPS + i] = row_tab[2 * ch + wy * ky + i];
            }
            const int lo = min(aug_wave_min(y0), in_h), hi = aug_wave_max(y1);
            const int rows = min(max(hi - lo, 0), AUG_ROWS);
            if (lane < ny) {
                rymin[lane] = y0 - lo;
                rn[lane] = max(min(n, rows - (y0 - lo)), 0);
            }
            if (lane == 0) { rect[2] = lo; rect[3] = rows; }
        } else if (ctab) {
            const int i = t - 128;                                           // 0 .. 127
            for (int k = i; k < 192; k += 128) reinterpret_cast<int*>(lut)[k] = ctab[k];
            for (int k = i; k < 256; k += 128) {
                sdiv[k] = ctab[192 + k];
                hdiv[k] = ctab[448 + k];
            }
        }
    }
    __syncthreads();

    if (inside) {
        const int sx0 = rect[0], npx = rect[1], sy0 = rect[2], rows = rect[3];
        // ---- 2. the source rectangle -> LDS -----------------------------------------------------------------------------------------
        const int nbytes = npx * 3;
        for (int idx = t; idx < rows * (AUG_RAW / 16); idx += AUG_THREADS) {
            const int r = idx / (AUG_RAW / 16), c = idx - r * (AUG_RAW / 16);
            const unsigned char* p = frame + ((size_t)(sy0 + r) * in_w + sx0) * 3;
            const int a = (int)((uintptr_t)p & 15);
            if (c == 0) shift[r] = (unsigned char)a;
            if (c * 16 >= a + nbytes) continue;
            const unsigned char* q = p - a + c * 16;
            if (q >= frame && q + 16 <= frame_end) {
                *reinterpret_cast<uint4*>(&raw[r][c * 16]) = *reinterpret_cast<const uint4*>(q);
            } else {
                for (int i = 0; i < 16; ++i) raw[r][c * 16 + i] = (q + i >= frame && q + i < frame_end) ? q[i] : 0;
            }
        }
        __syncthreads();
        // ---- 3. horizontal pass -----------------------------------------------------------------------------------------------------
        for (int idx = t; idx < rows * AUG_TW; idx += AUG_THREADS) {
            const int r = idx >> 6, j = idx & 63;
            if (j >= nx) continue;
            const unsigned char* p = &raw[r][shift[r] + cxmin[j] * 3];
            const int n = cn[j];
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
            for (int i = 0; i < n; ++i) {
                const int k = ck[j * AUG_TAPS + i];
                a0 += p[3 * i] * k;
                a1 += p[3 * i + 1] * k;
                a2 += p[3 * i + 2] * k;
            }
            mid[r][j * 3] = (unsigned char)aug_clip8(a0);
            mid[r][j * 3 + 1] = (unsigned char)aug_clip8(a1);
            mid[r][j * 3 + 2] = (unsigned char)aug_clip8(a2);
        }
        __syncthreads();
    }

    // ---- 4. vertical pass, colour, store --------------------------------------------------------------------------------------------
    const int i = t >> 4, j0 = (t & 15) * 4;
    const int oy = ty0 + i, ox0 = tx0 + j0;
    if (oy >= out_h || ox0 >= out_w) return;
    unsigned px[3] = {0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = j0 + q;
        int c0 = pad, c1 = pad, c2 = pad;
        if (i < ny && j < nx) {
            const int y = rymin[i], n = rn[i];
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
            for (int k = 0; k < n; ++k) {
                const int w = rk[i * AUG_TAPS + k];
                a0 += mid[y + k][j * 3] * w;
                a1 += mid[y + k][j * 3 + 1] * w;
                a2 += mid[y + k][j * 3 + 2] * w;
            }
            c0 = aug_clip8(a0); c1 = aug_clip8(a1); c2 = aug_clip8(a2);
            if (ctab) aug_colour(c0, c1, c2, cflags, hue, lut, sdiv, hdiv);
        }
        px[0] |= (unsigned)(c0 & 255) << (8 * q);
        px[1] |= (unsigned)(c1 & 255) << (8 * q);
        px[2] |= (unsigned)(c2 & 255) << (8 * q);
    }
    const size_t plane = (size_t)out_h * out_w;
    unsigned char* o = dst + (size_t)f * 3 * plane + (size_t)oy * out_w + ox0;
    const bool word = (out_w & 3) == 0 && ((uintptr_t)dst & 3) == 0;         // then every plane and every row start on a word
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (word) {
            *reinterpret_cast<unsigned*>(o + c * plane) = px[c];
        } else {
            for (int q = 0; q < 4 && ox0 + q < out_w; ++q) o[c * plane + q] = (unsigned char)(px[c] >> (8 * q));
        }
    }
}

// ---- labels: a gather through the nearest index tables ------------------------------------------------------------------------------------
// Block (64, 4): a thread owns four consecutive output pixels of one row and stores one int4 per map (single ints at a ragged edge).
template <typename L>
__global__ __launch_bounds__(256) void augment_labels_kernel(const unsigned char* __restrict__ pan, const L* __restrict__ label, int in_h, int in_w,
                                                             const int* __restrict__ pan_col, const int* __restrict__ pan_row,
                                                             const int* __restrict__ lab_col, const int* __restrict__ lab_row, int cw, int ch,
                                                             int flip, int out_h, int out_w, int ignore_label, int* __restrict__ pan_out,
                                                             int* __restrict__ label_out) {
    const int ox0 = (blockIdx.x * 64 + threadIdx.x) * 4, oy = blockIdx.y * 4 + threadIdx.y;
    if (oy >= out_h || ox0 >= out_w) return;
    int ids[4], labs[4];
    const bool row_in = oy < ch;
    const int pr = row_in ? min(max(pan_row[oy], 0), in_h - 1) : 0;
    const int lr = row_in && label ? min(max(lab_row[oy], 0), in_h - 1) : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ox = ox0 + q;
        ids[q] = 0;                                                          // VOID in the padding
        labs[q] = ignore_label;
        if (row_in && ox < cw && ox < out_w) {
            const int wx = flip ? cw - 1 - ox : ox;
            const int pc = min(max(pan_col[wx], 0), in_w - 1);
            const unsigned char* p = pan + ((size_t)pr * in_w + pc) * 3;
            ids[q] = (int)p[0] + 256 * (int)p[1] + 65536 * (int)p[2];
            if (label) labs[q] = (int)label[(size_t)lr * in_w + min(max(lab_col[wx], 0), in_w - 1)];
        }
    }
    const size_t at = (size_t)oy * out_w + ox0;
    const bool vec = (out_w & 3) == 0;
    if (vec && ((uintptr_t)pan_out & 15) == 0) {
        *reinterpret_cast<int4*>(pan_out + at) = make_int4(ids[0], ids[1], ids[2], ids[3]);
    } else {
        for (int q = 0; q < 4 && ox0 + q < out_w; ++q) pan_out[at + q] = ids[q];
    }
    if (!label_out) return;
    if (vec && ((uintptr_t)label_out & 15) == 0) {
        *reinterpret_cast<int4*>(label_out + at) = make_int4(labs[0], labs[1], labs[2], labs[3]);
    } else {
        for (int q = 0; q < 4 && ox0 + q < out_w; ++q) label_out[at + q] = labs[q];
    }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------------
static inline bool aug_aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

static inline bool aug_geometry_ok(int in_h, int in_w, int rs_h, int rs_w, int x0, int y0, int cw, int ch, int out_h, int out_w) {
    return in_h >= 1 && in_w >= 1 && (int64_t)in_h * in_w * 3 <= 0x7fffffff && rs_h >= 1 && rs_w >= 1 && rs_h <= 65536 && rs_w <= 65536 &&
           cw >= 1 && ch >= 1 && x0 >= 0 && y0 >= 0 && (int64_t)x0 + cw <= rs_w && (int64_t)y0 + ch <= rs_h &&      // the window lies inside
           out_h >= 1 && out_w >= 1 && out_h <= 65536 && out_w <= 65536;
}

extern "C" int uenc_augment_tile_fits(int in_h, int in_w, int rs_h, int rs_w, int kx, int ky) {
    if (in_h < 1 || in_w < 1 || rs_h < 1 || rs_w < 1 || kx < 1 || ky < 1 || kx > AUG_TAPS || ky > AUG_TAPS) return 0;
    // a tile's taps: (tile - 1) steps of the scale between the first and the last centre, plus one kernel width (2 * support + 1 <= k)
    const double span_x = (AUG_TW - 1) * ((double)in_w / rs_w) + kx + 1, span_y = (AUG_TH - 1) * ((double)in_h / rs_h) + ky + 1;
    return span_x <= (double)AUG_PIX && span_y <= (double)AUG_ROWS;
}

extern "C" int uenc_augment_image(const unsigned char* src, long frame_stride, int F, int in_h, int in_w, int rs_h, int rs_w, int x0, int y0,
                                  int cw, int ch, const int* col_tab, int kx, const int* row_tab, int ky, const int* colour_tab,
                                  int colour_flags, int hue, int flip, int out_h, int out_w, int pad_value, unsigned char* dst,
                                  hipStream_t stream) {
    UENC_CHECK_ARG(src && col_tab && row_tab && dst && aug_aligned4(col_tab) && aug_aligned4(row_tab) && aug_aligned4(colour_tab));
    UENC_CHECK_ARG(F >= 1 && F <= 65535 && aug_geometry_ok(in_h, in_w, rs_h, rs_w, x0, y0, cw, ch, out_h, out_w));
    UENC_CHECK_ARG(frame_stride >= (long)in_h * in_w * 3 && (flip == 0 || flip == 1) && pad_value >= 0 && pad_value <= 255);
    UENC_CHECK_ARG(colour_flags >= 0 && colour_flags < 16 && hue > -180 && hue < 180 && (colour_tab || colour_flags == 0));
    UENC_CHECK_ARG(uenc_augment_tile_fits(in_h, in_w, rs_h, rs_w, kx, ky));          // the plan's LDS tile must fit: no fallback
    const dim3 grid((out_w + AUG_TW - 1) / AUG_TW, (out_h + AUG_TH - 1) / AUG_TH, F);
    UENC_CHECK_ARG(grid.y <= 65535);
    hipLaunchKernelGGL(augment_image_kernel, grid, dim3(AUG_THREADS), 0, stream, src, frame_stride, in_h, in_w, col_tab, kx, row_tab, ky, cw, ch,
                       colour_tab, colour_flags, hue, flip, out_h, out_w, pad_value, dst);
    UENC_LAUNCH_RET();
}

extern "C" int uenc_augment_labels(const unsigned char* pan, const void* label, int label_bytes, int in_h, int in_w, int rs_h, int rs_w, int x0,
                                   int y0, int cw, int ch, const int* pan_col, const int* pan_row, const int* lab_col, const int* lab_row,
                                   int flip, int out_h, int out_w, int ignore_label, int* pan_out, int* label_out, hipStream_t stream) {
    UENC_CHECK_ARG(pan && pan_col && pan_row && pan_out && aug_aligned4(pan_col) && aug_aligned4(pan_row) && aug_aligned4(pan_out));
    UENC_CHECK_ARG(aug_geometry_ok(in_h, in_w, rs_h, rs_w, x0, y0, cw, ch, out_h, out_w) && (flip == 0 || flip == 1));
    UENC_CHECK_ARG((label == nullptr) == (label_out == nullptr));
    if (label) {
        UENC_CHECK_ARG(lab_col && lab_row && aug_aligned4(lab_col) && aug_aligned4(lab_row) && aug_aligned4(label_out));
        UENC_CHECK_ARG(label_bytes == 1 || (label_bytes == 4 && aug_aligned4(label)));
    }
    const dim3 grid((out_w + 255) / 256, (out_h + 3) / 4), block(64, 4);
    UENC_CHECK_ARG(grid.y <= 65535);
#define AUG_LABELS(L)                                                                                                                       \
    hipLaunchKernelGGL(augment_labels_kernel<L>, grid, block, 0, stream, pan, (const L*)label, in_h, in_w, pan_col, pan_row, lab_col, lab_row, cw, \
                       ch, flip, out_h, out_w, ignore_label, pan_out, label_out)
    if (label_bytes == 4) AUG_LABELS(int);
    else AUG_LABELS(unsigned char);
#undef AUG_LABELS
    UENC_LAUNCH_RET();
}
