// niti_dataset.hip -- the batch gather of the device-resident dataset: n entries of an order
// (index[], optional xform[]) out of data[count][C][H][W] / labels[count] into one contiguous
// uint8 batch out[n][C][H][W] with labels_out[n], the form every niti_model_*_images step takes.
//
// Entry i, s = index[i].  s outside [0, count) (the host admits only -1 there: the padding of a
// last partial batch): a zero image with label -1.  Otherwise, with dx = (int8)(xform & 0xff),
// dy = (int8)(xform >> 8 & 0xff), flip = xform >> 16 & 1 (all 0 without an xform array):
//   out[i][ch][y][x] = data[s][ch][y + dy][(flip ? W - 1 - x : x) + dx], 0 outside the image
// -- zero-pad by P, crop at offset (P + dy, P + dx), then mirror.  |dx| >= W or |dy| >= H is legal
// and gives a zero image.
//
// Three kernels, each a grid-stride loop of plain loads and stores (no atomics, no LDS), chosen
// from the geometry and the pointers' alignment:
//   copy16   no xform, C*H*W % 16 == 0: a 16-byte load and store per lane.
//   xform<D> W % 4 == 0: a lane owns D = 4 (W % 16 == 0, one 16-byte store) or D = 1 output dwords
//            of one row.  Their source span starts at byte a = x0 + dx of the row (a = W - 4*D -
//            x0 + dx mirrored): the lane loads the D + 1 aligned dwords from a >> 2 on, funnel-
//            shifts each neighbouring pair by a & 3 bytes (v_alignbyte_b32) and, mirrored,
//            reverses bytes and dword order (v_perm_b32).  As W % 4 == 0 an aligned dword lies
//            wholly inside or wholly outside the row: the zero fill is the load's own mask, and no
//            address outside [row, row + W) is formed into a load.
//   bytes    anything else (W % 4 != 0, images that start unaligned): one byte per lane.
// The label is written by the lane that owns an image's first unit.
//
// batch_gather_resize (further down) is the gather of an order that carries crop windows: it crops,
// resizes bilinearly to the dataset's output size and mirrors, in one launch.
#include <algorithm>

#include "niti_kernels.hpp"

namespace niti {

namespace {

constexpr int GATHER_MAX_BLOCKS = 2048;

struct GatherArgs {
    const uint8_t* data;
    const int32_t* labels;
    int64_t count;
    int c, h, w;
    const int32_t* index;
    const int32_t* xform;  // may be null
    int n;
    uint8_t* out;
    int32_t* labels_out;
};

__device__ inline bool entry_ok(const GatherArgs& a, int i, int64_t* s) {
    *s = a.index[i];
    return *s >= 0 && *s < a.count;
}

__global__ void __launch_bounds__(256) gather_copy16_kernel(GatherArgs a) {
    const int64_t per = (int64_t)a.c * a.h * a.w / 16;  // 16-byte units per image
    const int64_t total = per * a.n;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(q / per);
        const int64_t u = q - (int64_t)i * per;
        int64_t s;
        const bool ok = entry_ok(a, i, &s);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ok) v = reinterpret_cast<const uint4*>(a.data)[s * per + u];
        reinterpret_cast<uint4*>(a.out)[q] = v;
        if (u == 0) a.labels_out[i] = ok ? a.labels[s] : -1;
    }
}

template <int D>
__global__ void __launch_bounds__(256) gather_xform_kernel(GatherArgs a) {
    const int wd = a.w / 4;                 // aligned dwords per row
    const int upr = wd / D;                 // units per row
    const int rows = a.c * a.h;
    const int64_t per = (int64_t)rows * upr;  // units per image
    const int64_t total = per * a.n;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(q / per);
        const int r = (int)(q - (int64_t)i * per);
        const int row = r / upr;  // ch * H + y
        const int x0 = (r - row * upr) * (4 * D);
        int64_t s;
        const bool ok = entry_ok(a, i, &s);
        const uint32_t t = (uint32_t)a.xform[i];
        const int dx = (int)(int8_t)(t & 0xff), dy = (int)(int8_t)((t >> 8) & 0xff);
        const bool flip = (t >> 16) & 1;
        const int ch = row / a.h;
        const int ys = row - ch * a.h + dy;
        uint32_t o[D];
#pragma unroll
        for (int k = 0; k < D; ++k) o[k] = 0;
        if (ok && ys >= 0 && ys < a.h) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(a.data) + (s * rows + (int64_t)ch * a.h + ys) * wd;
            const int b = (flip ? a.w - 4 * D - x0 : x0) + dx;  // first source byte of the span, in the row
            const int lo = b >> 2;                              // (arithmetic: floor)
            const uint32_t sh = (uint32_t)(b & 3);
            uint32_t d[D + 1];
#pragma unroll
            for (int k = 0; k <= D; ++k) {
                const int j = lo + k;
                d[k] = (j >= 0 && j < wd && (k < D || sh != 0)) ? src[j] : 0u;
            }
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const uint32_t v = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);  // source bytes b + 4k .. + 3
                if (flip)
                    o[D - 1 - k] = __builtin_amdgcn_perm(0u, v, 0x00010203u);  // byte reverse
                else
                    o[k] = v;
            }
        }
        uint32_t* dst = reinterpret_cast<uint32_t*>(a.out) + q * D;
        if constexpr (D == 4) {
            *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) dst[k] = o[k];
        }
        if (r == 0) a.labels_out[i] = ok ? a.labels[s] : -1;
    }
}

__global__ void __launch_bounds__(256) gather_bytes_kernel(GatherArgs a) {
    const int hw = a.h * a.w;
    const int64_t per = (int64_t)a.c * hw;
    const int64_t total = per * a.n;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(q / per);
        const int r = (int)(q - (int64_t)i * per);
        int64_t s;
        const bool ok = entry_ok(a, i, &s);
        const uint32_t t = a.xform ? (uint32_t)a.xform[i] : 0u;
        const int dx = (int)(int8_t)(t & 0xff), dy = (int)(int8_t)((t >> 8) & 0xff);
        const bool flip = (t >> 16) & 1;
        const int ch = r / hw;
        const int y = (r - ch * hw) / a.w;
        const int x = r - ch * hw - y * a.w;
        const int xs = (flip ? a.w - 1 - x : x) + dx, ys = y + dy;
        uint8_t v = 0;
        if (ok && xs >= 0 && xs < a.w && ys >= 0 && ys < a.h) v = a.data[s * per + (int64_t)ch * hw + ys * a.w + xs];
        a.out[q] = v;
        if (r == 0) a.labels_out[i] = ok ? a.labels[s] : -1;
    }
}

template <class K>
hipError_t launch(K kernel, int64_t units, const GatherArgs& a, hipStream_t st) {
    const int64_t blocks = std::min<int64_t>((units + 255) / 256, GATHER_MAX_BLOCKS);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---- crop-and-resize gather (batch_gather_resize; the definition is in include/niti_hip.h)
// A block owns one entry's output rows [y_lo, y_lo + nrows) x columns [x_lo, x_lo + ncols), all
// channels.  It builds the positions of its columns (mirrored: the table is simply filled in
// reverse) and rows once in LDS -- the only integer divisions -- and then walks its units of D
// adjacent pixels of one row, D = 16 (one 16-byte store), 4 (one dword store) or 1: four source
// bytes per pixel, two 8-bit lerps, one pack.  The walks step (channel,) row and unit by the
// block's 256 threads with carries, not divisions.
// Where the source rows the block needs of one channel fit RS_TILE bytes of LDS they are staged
// there first, channel by channel, with aligned dword loads (a byte load per sample costs a vector
// memory instruction each: the measured bound of the direct form), and the samples are LDS byte
// reads; otherwise (a steep downscale) the samples are byte loads through the cache.
// The window words are clamped into the stored image before use, so every sample address lies
// inside data[s][ch] whatever they hold; a staged dword is loaded whole only where it lies inside
// data[0 .. count), byte by byte at the dataset's two ends.
constexpr int RS_COLS = 2048;     // output columns per block at most (a multiple of 16)
constexpr int RS_ROWS = 64;       // output rows per block at most
constexpr int RS_PIXELS = 16384;  // output pixels per block aimed for
constexpr int RS_TILE = 24576;    // bytes of LDS for one channel's staged source rows (4 blocks per CU)

struct ResizeArgs {
    const uint8_t* data;
    const int32_t* labels;
    int64_t count;
    int c, h, w;
    const int32_t* index;
    const int32_t* xform;   // may be null; only the flip bit is read
    const int32_t* window;  // [n][4] = x0, y0, cw, ch
    int n, oh, ow;
    uint8_t* out;
    int32_t* labels_out;
    int rows, strips, chunks;  // output rows per block; row strips and column chunks per entry
};

// position of output coordinate o in a window of cn pixels, in 1/256 px: corner to corner
__device__ inline uint32_t resize_pos(uint32_t o, uint32_t n_out, uint32_t cn) {
    return n_out == 1 ? 0u : (2u * o * (cn - 1u) * 256u + (n_out - 1u)) / (2u * (n_out - 1u));
}

// One unit: D adjacent pixels from the column records colrec[0 .. D) and the source rows s0 / s1,
// functions of the column relative to the window's first, stored at dst.
template <int D, class S0, class S1>
__device__ inline void resize_unit(const uint32_t* colrec, int cw, uint32_t fy, bool ok, S0 s0, S1 s1, uint8_t* dst) {
    uint32_t o[(D + 3) / 4];
#pragma unroll
    for (int k = 0; k < (D + 3) / 4; ++k) o[k] = 0;
    if (ok) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const uint32_t px = colrec[k];
            const int ix = (int)(px >> 8), ix1 = min(ix + 1, cw - 1);
            const uint32_t fx = px & 255u;
            const uint32_t top = (256u - fx) * s0(ix) + fx * s0(ix1);
            const uint32_t bot = (256u - fx) * s1(ix) + fx * s1(ix1);
            o[k / 4] |= ((top * (256u - fy) + bot * fy + 32768u) >> 16) << (8 * (k % 4));
        }
    }
    if constexpr (D == 16)
        *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
    else if constexpr (D == 4)
        *reinterpret_cast<uint32_t*>(dst) = o[0];
    else
        *dst = (uint8_t)o[0];
}

template <int D>
__global__ void __launch_bounds__(256) gather_resize_kernel(ResizeArgs a) {
    __shared__ alignas(16) uint32_t col[RS_COLS];
    __shared__ uint32_t row[RS_ROWS];
    __shared__ alignas(16) uint32_t tile[RS_TILE / 4];
    const int tid = threadIdx.x;
    const int per = a.strips * a.chunks;
    const int i = blockIdx.x / per;
    const int rem = blockIdx.x - i * per;
    const int strip = rem / a.chunks;
    const int y_lo = strip * a.rows, x_lo = (rem - strip * a.chunks) * RS_COLS;
    const int nrows = min(a.rows, a.oh - y_lo), ncols = min(RS_COLS, a.ow - x_lo);
    const int64_t s = a.index[i];
    const bool ok = s >= 0 && s < a.count;
    if (rem == 0 && tid == 0) a.labels_out[i] = ok ? a.labels[s] : -1;
    int x0 = 0, y0 = 0, cw = 1, chh = 1;
    if (ok) {
        const int32_t* wd = a.window + (int64_t)i * 4;
        cw = min(max(wd[2], 1), a.w);
        chh = min(max(wd[3], 1), a.h);
        x0 = min(max(wd[0], 0), a.w - cw);
        y0 = min(max(wd[1], 0), a.h - chh);
        const bool flip = a.xform != nullptr && ((a.xform[i] >> 16) & 1);
        for (int j = tid; j < ncols; j += 256) {
            const int x = x_lo + j;
            col[j] = resize_pos((uint32_t)(flip ? a.ow - 1 - x : x), (uint32_t)a.ow, (uint32_t)cw);
        }
        for (int j = tid; j < nrows; j += 256) row[j] = resize_pos((uint32_t)(y_lo + j), (uint32_t)a.oh, (uint32_t)chh);
    }
    __syncthreads();
    const int upr = ncols / D;  // units per row (ncols % D == 0: the host picks D so)
    const int64_t plane = (int64_t)a.h * a.w;
    // the source rows [sy0, sy0 + srows) x columns [sx0, sx0 + swidth) of the window this block
    // samples (positions are monotonic: the extremes sit at the tables' ends)
    int sy0 = 0, sx0 = 0, srows = 0, swidth = 0, pitch = 4;
    bool staged = false;
    if (ok) {
        sy0 = (int)(row[0] >> 8);
        srows = min((int)(row[nrows - 1] >> 8) + 1, chh - 1) - sy0 + 1;
        const int ixa = (int)(col[0] >> 8), ixb = (int)(col[ncols - 1] >> 8);
        sx0 = min(ixa, ixb);
        swidth = min(max(ixa, ixb) + 1, cw - 1) - sx0 + 1;
        pitch = (swidth + 6) & ~3;  // up to 3 bytes ahead of an unaligned row, whole dwords
        staged = (int64_t)srows * pitch <= RS_TILE;
    }
    if (staged) {  // (uniform over the block)
        const uint8_t* tile8 = reinterpret_cast<const uint8_t*>(tile);
        const int pdw = pitch / 4;
        const uintptr_t lo = (uintptr_t)a.data, hi = lo + (uintptr_t)(a.count * a.c * plane);
        for (int ch = 0; ch < a.c; ++ch) {
            // tile row 0, window column sx0
            const uint8_t* src = a.data + (s * a.c + ch) * plane + (int64_t)(y0 + sy0) * a.w + x0 + sx0;
            int j = tid % pdw, sr = tid / pdw;
            const int dj = 256 % pdw, dsr = 256 / pdw;
            while (sr < srows) {
                const uint8_t* rp = src + (int64_t)sr * a.w;
                const int lead = (int)((uintptr_t)rp & 3);
                if (4 * j < lead + swidth) {
                    const uint8_t* g = rp - lead + 4 * j;  // (4-byte aligned)
                    uint32_t v = 0;
                    if ((uintptr_t)g >= lo && (uintptr_t)g + 4 <= hi) {
                        v = *reinterpret_cast<const uint32_t*>(g);
                    } else {
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                            if ((uintptr_t)(g + b) >= lo && (uintptr_t)(g + b) < hi) v |= (uint32_t)g[b] << (8 * b);
                    }
                    tile[sr * pdw + j] = v;
                }
                j += dj;
                sr += dsr;
                if (j >= pdw) {
                    j -= pdw;
                    ++sr;
                }
            }
            __syncthreads();
            int cu = tid % upr, r = tid / upr;
            const int dcu = 256 % upr, dr = 256 / upr;
            while (r < nrows) {
                const uint32_t py = row[r];
                const int ty = (int)(py >> 8) - sy0, ty1 = min(ty + 1, srows - 1);
                // byte of window column ix in tile row t: t * pitch + (its row's lead) + ix - sx0
                const int b0 = ty * pitch + (int)((uintptr_t)(src + (int64_t)ty * a.w) & 3) - sx0;
                const int b1 = ty1 * pitch + (int)((uintptr_t)(src + (int64_t)ty1 * a.w) & 3) - sx0;
                resize_unit<D>(
                    col + cu * D, cw, py & 255u, true, [&](int ix) { return (uint32_t)tile8[b0 + ix]; },
                    [&](int ix) { return (uint32_t)tile8[b1 + ix]; },
                    a.out + (((int64_t)i * a.c + ch) * a.oh + (y_lo + r)) * a.ow + x_lo + cu * D);
                cu += dcu;
                r += dr;
                if (cu >= upr) {
                    cu -= upr;
                    ++r;
                }
            }
            __syncthreads();  // (the next channel overwrites the tile)
        }
        return;
    }
    int cu = tid % upr, r = (tid / upr) % nrows, ch = tid / upr / nrows;
    const int dcu = 256 % upr, dr = (256 / upr) % nrows, dch = 256 / upr / nrows;
    while (ch < a.c) {
        const uint32_t py = ok ? row[r] : 0u;
        const int iy = (int)(py >> 8), iy1 = min(iy + 1, chh - 1);
        const uint8_t* p0 = a.data;
        const uint8_t* p1 = a.data;
        if (ok) {
            p0 = a.data + (s * a.c + ch) * plane + (int64_t)(y0 + iy) * a.w + x0;
            p1 = a.data + (s * a.c + ch) * plane + (int64_t)(y0 + iy1) * a.w + x0;
        }
        resize_unit<D>(
            col + cu * D, cw, py & 255u, ok, [&](int ix) { return (uint32_t)p0[ix]; },
            [&](int ix) { return (uint32_t)p1[ix]; },
            a.out + (((int64_t)i * a.c + ch) * a.oh + (y_lo + r)) * a.ow + x_lo + cu * D);
        cu += dcu;
        r += dr;
        ch += dch;
        if (cu >= upr) {
            cu -= upr;
            ++r;
        }
        if (r >= nrows) {
            r -= nrows;
            ++ch;
        }
    }
}

}  // namespace

bool resize_size_ok(int in, int out) { return in >= 1 && out >= 1 && (int64_t)(out - 1) * (in - 1) < (int64_t(1) << 22); }

hipError_t batch_gather_resize(const uint8_t* data, const int32_t* labels, int64_t count, int c, int h, int w,
                               const int32_t* index, const int32_t* xform, const int32_t* window, int n, int oh,
                               int ow, uint8_t* out, int32_t* labels_out, hipStream_t st) {
    if (!data || !labels || !index || !window || !out || !labels_out || count <= 0 || c <= 0 || n <= 0 ||
        !resize_size_ok(h, oh) || !resize_size_ok(w, ow))
        return hipErrorInvalidValue;
    if ((int64_t)c * h * w > INT32_MAX || (int64_t)c * oh * ow > INT32_MAX) return hipErrorInvalidValue;
    ResizeArgs a{data, labels, count, c, h, w, index, xform, window, n, oh, ow, out, labels_out, 0, 0, 0};
    a.rows = (int)std::clamp<int64_t>(RS_PIXELS / ((int64_t)c * std::min(ow, RS_COLS)), 1, std::min(RS_ROWS, oh));
    a.strips = (oh + a.rows - 1) / a.rows;
    a.chunks = (ow + RS_COLS - 1) / RS_COLS;
    const int64_t blocks = (int64_t)n * a.strips * a.chunks;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(256);
    if (ow % 16 == 0 && ((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL(gather_resize_kernel<16>, grid, block, 0, st, a);
    else if (ow % 4 == 0 && ((uintptr_t)out & 3) == 0)
        hipLaunchKernelGGL(gather_resize_kernel<4>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(gather_resize_kernel<1>, grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t batch_gather(const uint8_t* data, const int32_t* labels, int64_t count, int c, int h, int w,
                        const int32_t* index, const int32_t* xform, int n, uint8_t* out, int32_t* labels_out,
                        hipStream_t st) {
    if (!data || !labels || !index || !out || !labels_out || count <= 0 || c <= 0 || h <= 0 || w <= 0 || n <= 0)
        return hipErrorInvalidValue;
    const int64_t per = (int64_t)c * h * w;
    if (per > INT32_MAX) return hipErrorInvalidValue;  // (an image's inner offsets are int)
    const GatherArgs a{data, labels, count, c, h, w, index, xform, n, out, labels_out};
    const uintptr_t al = (uintptr_t)data | (uintptr_t)out;
    if (xform == nullptr && per % 16 == 0 && (al & 15) == 0) return launch(gather_copy16_kernel, per / 16 * n, a, st);
    if (xform != nullptr && w % 16 == 0 && (al & 15) == 0) return launch(gather_xform_kernel<4>, per / 16 * n, a, st);
    if (xform != nullptr && w % 4 == 0 && (al & 3) == 0) return launch(gather_xform_kernel<1>, per / 4 * n, a, st);
    return launch(gather_bytes_kernel, per * n, a, st);
}

}  // namespace niti
