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

}  // namespace

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
