// niti_pointwise.hip -- the rest of the step beside the GEMMs: the max pool and its gradients (NITI_Maxpool_Int8.cpp,
// NITI_CPUPoolGrad_Int8.cpp, with NITI_CPUReluGrad_Int8 fused), relu_grad, the loss gradient in its three forms
// (NITI_LOSS_Grad: the rows of loss_rows16 in niti_sgd.hpp, the wide rows here, and the launch shared with the P16
// conversion jobs of niti_wgrad.hip), grad_exponent, and every layout conversion between the reference's tensors
// (NCHW, NC4HW4, OIHW) and the kernels' (NHWC16, CHWN16, OHWI16, IHWO16) as launch_map functors (niti_map.hpp).
// Nothing here knows the GEMM's planning or state; the entry points are declared in niti_kernels.hpp.
#include <algorithm>

#include "niti_device.hpp"
#include "niti_kernels.hpp"
#include "niti_sgd.hpp"
#include "niti_map.hpp"

namespace niti {

// =====================================================================================
// The rest of the step: pool / relu-grad / loss-grad
// =====================================================================================

// NITI_Maxpool_Int8.cpp:24-72 (kernel clipped to the input); one thread per 16 channels (32-bit
// index math: the host keeps the thread count below 2^31).  With `arg`, each window's first-max
// position (ky * k + kx, in NITI_CPUPoolGrad_Int8.cpp:21-77's order) goes there too: the first
// element equal to the max is the first one >= it, the backward pass's choice (on a map smaller
// than the kernel the two windows differ: see below).
__global__ void maxpool_kernel(const int8_t* __restrict__ x, int n, int h, int w, int cp, int k, int s, int p,
                               int8_t* __restrict__ y, int oh, int ow, int8_t* __restrict__ arg) {
    const uint32_t groups = cp / 16;
    const uint32_t total = (uint32_t)n * oh * ow * groups;
    const int kh = k < h ? k : h, kw = k < w ? k : w;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        uint32_t r = t;
        const int gi = (int)(r % groups);
        r /= groups;
        const int ox = (int)(r % (uint32_t)ow);
        r /= (uint32_t)ow;
        const int oy = (int)(r % (uint32_t)oh);
        const int b = (int)(r / (uint32_t)oh);
        const int sx0 = ox * s - p, sy0 = oy * s - p;
        v16c m, a;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            m[j] = (signed char)-128;
            a[j] = (signed char)-1;
        }
        for (int yy = max(0, -sy0); yy < min(kh, h - sy0); ++yy)
            for (int xx = max(0, -sx0); xx < min(kw, w - sx0); ++xx) {
                const v16c v = *(const v16c*)(x + (((int64_t)b * h + sy0 + yy) * w + sx0 + xx) * cp + gi * 16);
                const signed char pos = (signed char)(yy * k + xx);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const bool take = a[j] < 0 || v[j] > m[j];
                    m[j] = take ? v[j] : m[j];
                    a[j] = take ? pos : a[j];
                }
            }
        *(v16c*)(y + (int64_t)t * 16) = m;
        if (arg != nullptr && (kh < k || kw < k)) {
            // A map smaller than the kernel: the reference clips the forward's window (above) but not
            // the gradient's scan, which takes the first in-image element >= the max of the whole
            // k x k window (NITI_CPUPoolGrad_Int8.cpp:21-77).  That element is what arg records.
#pragma unroll
            for (int j = 0; j < 16; ++j) a[j] = (signed char)-1;
            for (int yy = max(0, -sy0); yy < min(k, h - sy0); ++yy)
                for (int xx = max(0, -sx0); xx < min(k, w - sx0); ++xx) {
                    const v16c v = *(const v16c*)(x + (((int64_t)b * h + sy0 + yy) * w + sx0 + xx) * cp + gi * 16);
                    const signed char pos = (signed char)(yy * k + xx);
#pragma unroll
                    for (int j = 0; j < 16; ++j) a[j] = (a[j] < 0 && v[j] >= m[j]) ? pos : a[j];
                }
        }
        if (arg != nullptr) *(v16c*)(arg + (int64_t)t * 16) = a;
    }
}

hipError_t maxpool_nhwc16(const int8_t* x, int n, int h, int w, int cp, int k, int s, int p, int8_t* y, int oh, int ow,
                          hipStream_t st, int8_t* arg) {
    const int64_t total = (int64_t)n * oh * ow * (cp / 16);
    if (total >= ((int64_t)1 << 31) || cp % 16 != 0) return hipErrorInvalidValue;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, n, h, w, cp, k, s, p, y, oh, ow, arg);
    return hipGetLastError();
}

// NITI_CPUPoolGrad_Int8.cpp:21-77 in gather form: input pixel (iy,ix) receives, from every
// window containing it, dy if it is that window's first (ky,kx) element with x >= max.
// Optionally fused NITI_CPUReluGrad_Int8 (out = x > 0 ? dx : 0).
__global__ void maxpool_grad_kernel(const int8_t* __restrict__ x, const int8_t* __restrict__ y,
                                    const int8_t* __restrict__ dy, int n, int h, int w, int cp, int k, int s,
                                    int p, int oh, int ow, int relu, int8_t* __restrict__ dx) {
    const int groups = cp / 16;
    const int64_t total = (int64_t)n * h * w * groups;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t r = t;
        const int gi = (int)(r % groups);
        r /= groups;
        const int ix = (int)(r % w);
        r /= w;
        const int iy = (int)(r % h);
        const int b = (int)(r / h);
        const v16c xv = *(const v16c*)(x + (((int64_t)b * h + iy) * w + ix) * cp + gi * 16);
        v16c acc;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0;
        // windows (oy, ox) with oy*s - p <= iy < oy*s - p + k
        const int oy_lo = max(0, (iy + p - k + s) / s), oy_hi = min(oh - 1, (iy + p) / s);
        const int ox_lo = max(0, (ix + p - k + s) / s), ox_hi = min(ow - 1, (ix + p) / s);
        for (int oy = oy_lo; oy <= oy_hi; ++oy)
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const int sy0 = oy * s - p, sx0 = ox * s - p;
                if (iy < sy0 || iy >= sy0 + k || ix < sx0 || ix >= sx0 + k) continue;
                const int64_t po = (((int64_t)b * oh + oy) * ow + ox) * cp + gi * 16;
                const v16c mv = *(const v16c*)(y + po);
                const v16c dv = *(const v16c*)(dy + po);
                // is (iy,ix) the first element >= max in this window, per channel?
                unsigned first = 0xffffu;
                for (int ky = 0; ky < k; ++ky) {
                    const int sy = sy0 + ky;
                    if (sy < 0 || sy >= h) continue;
                    for (int kx = 0; kx < k; ++kx) {
                        const int sx = sx0 + kx;
                        if (sx < 0 || sx >= w) continue;
                        if (sy == iy && sx == ix) goto done;
                        {
                            const v16c ov = *(const v16c*)(x + (((int64_t)b * h + sy) * w + sx) * cp + gi * 16);
#pragma unroll
                            for (int j = 0; j < 16; ++j)
                                if (ov[j] >= mv[j]) first &= ~(1u << j);
                        }
                    }
                }
            done:
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (((first >> j) & 1u) && xv[j] >= mv[j]) acc[j] = (signed char)(acc[j] + dv[j]);
            }
        if (relu) {
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = xv[j] > 0 ? acc[j] : (signed char)0;
        }
        *(v16c*)(dx + (((int64_t)b * h + iy) * w + ix) * cp + gi * 16) = acc;
    }
}

// Non-overlapping windows (k == s, no padding, windows tile the input): one thread per window
// and 16 channels scans its k*k pixels once in the reference's (ky, kx) order.
__global__ void maxpool_grad_tiled_kernel(const int8_t* __restrict__ x, const int8_t* __restrict__ y,
                                          const int8_t* __restrict__ dy, int n, int h, int w, int cp, int k,
                                          int oh, int ow, int relu, int8_t* __restrict__ dx) {
    const int groups = cp / 16;
    const int64_t total = (int64_t)n * oh * ow * groups;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t r = t;
        const int gi = (int)(r % groups);
        r /= groups;
        const int ox = (int)(r % ow);
        r /= ow;
        const int oy = (int)(r % oh);
        const int b = (int)(r / oh);
        const int64_t po = (((int64_t)b * oh + oy) * ow + ox) * cp + gi * 16;
        const v16c mv = *(const v16c*)(y + po);
        const v16c dv = *(const v16c*)(dy + po);
        unsigned done = 0;
        for (int ky = 0; ky < k; ++ky)
            for (int kx = 0; kx < k; ++kx) {
                const int64_t pi = (((int64_t)b * h + oy * k + ky) * w + ox * k + kx) * cp + gi * 16;
                const v16c xv = *(const v16c*)(x + pi);
                v16c o;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const bool take = !((done >> j) & 1u) && xv[j] >= mv[j];
                    if (take) done |= 1u << j;
                    signed char d = take ? dv[j] : (signed char)0;
                    if (relu && xv[j] <= 0) d = 0;
                    o[j] = d;
                }
                *(v16c*)(dx + pi) = o;
            }
    }
}

hipError_t maxpool_relu_grad_nhwc16(const int8_t* x, const int8_t* y, const int8_t* dy, int n, int h, int w, int cp,
                                    int k, int s, int p, int oh, int ow, int relu, int8_t* dx, hipStream_t st) {
    if (k == s && p == 0 && oh * k == h && ow * k == w) {
        const int64_t total = (int64_t)n * oh * ow * (cp / 16);
        int64_t blocks = (total + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL(maxpool_grad_tiled_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, y, dy, n, h, w, cp,
                           k, oh, ow, relu, dx);
        return hipGetLastError();
    }
    const int64_t total = (int64_t)n * h * w * (cp / 16);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(maxpool_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, y, dy, n, h, w, cp, k, s, p,
                       oh, ow, relu, dx);
    return hipGetLastError();
}

// Overlapping windows in two passes over a caller workspace (the generic kernel above re-reads up
// to 8 x vectors per window for every input pixel).  Pass 1, per window and 16 channels: the
// position (ky * k + kx, in NITI_CPUPoolGrad_Int8.cpp's order, in-image elements only) of the
// first element >= the window max y.  Pass 2, per input pixel: the sum (int8, wrapping, as the
// reference's accumulation) of dy over the windows whose first max is this pixel, then the relu
// mask.  Results equal maxpool_grad_kernel's.
__global__ void maxpool_argmax_kernel(const int8_t* __restrict__ x, const int8_t* __restrict__ y, int n, int h, int w,
                                      int cp, int k, int s, int p, int oh, int ow, int8_t* __restrict__ arg) {
    const int groups = cp / 16;
    const int64_t total = (int64_t)n * oh * ow * groups;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t r = t;
        const int gi = (int)(r % groups);
        r /= groups;
        const int ox = (int)(r % ow);
        r /= ow;
        const int oy = (int)(r % oh);
        const int b = (int)(r / oh);
        const v16c mv = *(const v16c*)(y + t * 16);
        v16c a;
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = (signed char)-1;
        uint32_t open = 0xffffu;
        const int sy0 = oy * s - p, sx0 = ox * s - p;
        for (int ky = 0; ky < k && open; ++ky) {
            const int sy = sy0 + ky;
            if (sy < 0 || sy >= h) continue;
            for (int kx = 0; kx < k && open; ++kx) {
                const int sx = sx0 + kx;
                if (sx < 0 || sx >= w) continue;
                const v16c xv = *(const v16c*)(x + (((int64_t)b * h + sy) * w + sx) * cp + gi * 16);
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (((open >> j) & 1u) && xv[j] >= mv[j]) {
                        a[j] = (signed char)(ky * k + kx);
                        open &= ~(1u << j);
                    }
            }
        }
        *(v16c*)(arg + t * 16) = a;
    }
}

__global__ void maxpool_grad_gather_kernel(const int8_t* __restrict__ x, const int8_t* __restrict__ arg,
                                           const int8_t* __restrict__ dy, int n, int h, int w, int cp, int k, int s,
                                           int p, int oh, int ow, int relu, int8_t* __restrict__ dx,
                                           const int8_t* __restrict__ pooled) {
    const bool ymask = relu && pooled != nullptr;  // the relu mask from the window's pooled value
    const uint32_t groups = cp / 16;
    const uint32_t total = (uint32_t)n * h * w * groups;  // < 2^31 (host)
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        uint32_t r = t;
        const int gi = (int)(r % groups);
        r /= groups;
        const int ix = (int)(r % (uint32_t)w);
        r /= (uint32_t)w;
        const int iy = (int)(r % (uint32_t)h);
        const int b = (int)(r / (uint32_t)h);
        v16c acc;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0;
        const int oy_lo = max(0, (iy + p - k + s) / s), oy_hi = min(oh - 1, (iy + p) / s);
        const int ox_lo = max(0, (ix + p - k + s) / s), ox_hi = min(ow - 1, (ix + p) / s);
        for (int oy = oy_lo; oy <= oy_hi; ++oy)
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const int ky = iy - (oy * s - p), kx = ix - (ox * s - p);
                if (ky < 0 || ky >= k || kx < 0 || kx >= k) continue;
                const int64_t po = (((int64_t)b * oh + oy) * ow + ox) * cp + gi * 16;
                const v16c av = *(const v16c*)(arg + po);
                const v16c dv = *(const v16c*)(dy + po);
                v16c pv;
                if (ymask) pv = *(const v16c*)(pooled + po);
                const signed char me = (signed char)(ky * k + kx);
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (av[j] == me && (!ymask || pv[j] > 0)) acc[j] = (signed char)(acc[j] + dv[j]);
            }
        if (relu && !ymask) {
            const v16c xv = *(const v16c*)(x + (int64_t)t * 16);
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = xv[j] > 0 ? acc[j] : (signed char)0;
        }
        *(v16c*)(dx + (int64_t)t * 16) = acc;
    }
}

// The same gather for the 3x3 / 2 pad-1 pool with the relu mask from the pooled output (ResNet-18's
// stem): four bytes at a time per 32-bit word (first-max match, pooled > 0, wrapping int8 sum)
// instead of a byte loop -- the byte form is VALU-bound.  Pooled values are relu outputs (>= 0).
struct PoolGradGeom {
    FastDiv fg, fw, fh;  // by 16-channel groups, input width, input height
    int oh, ow;
    uint32_t total;
};
__global__ void __launch_bounds__(256) maxpool3_grad_pooled_kernel(const uint4* __restrict__ arg, const uint4* __restrict__ dy,
                                                                   const uint4* __restrict__ pooled, PoolGradGeom g,
                                                                   uint4* __restrict__ dx) {
    const uint32_t groups = g.fg.d, w = g.fw.d, h = g.fh.d;
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < g.total; t += gridDim.x * 256u) {
        const uint32_t r0 = fdiv(g.fg, t), gi = t - r0 * groups;
        const uint32_t r1 = fdiv(g.fw, r0), ix = r0 - r1 * w;
        const uint32_t b = fdiv(g.fh, r1), iy = r1 - b * h;
        uint32_t acc[4] = {0, 0, 0, 0};
        // windows oy with 2 oy - 1 <= iy <= 2 oy + 1 (ky = iy + 1 - 2 oy), likewise ox
        const int oy_lo = ((int)iy) >> 1, oy_hi = min(g.oh - 1, ((int)iy + 1) >> 1);
        const int ox_lo = ((int)ix) >> 1, ox_hi = min(g.ow - 1, ((int)ix + 1) >> 1);
        for (int oy = oy_lo; oy <= oy_hi; ++oy)
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const uint32_t me = (uint32_t)(((int)iy + 1 - 2 * oy) * 3 + ((int)ix + 1 - 2 * ox)) * 0x01010101u;
                const int64_t po = (((int64_t)b * g.oh + oy) * g.ow + ox) * groups + gi;
                const uint4 av = arg[po], dv = dy[po], pv = pooled[po];
                const uint32_t aw[4] = {av.x, av.y, av.z, av.w}, dw[4] = {dv.x, dv.y, dv.z, dv.w},
                               pw[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t d = aw[e] ^ me;  // 0 bytes: this pixel is the window's first max
                    const uint32_t hit = ~(((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d | 0x7f7f7f7fu);
                    const uint32_t pos = ((pw[e] & 0x7f7f7f7fu) + 0x7f7f7f7fu) & ~pw[e] & 0x80808080u;  // pooled > 0
                    const uint32_t c = dw[e] & (((hit & pos) >> 7) * 0xffu);
                    acc[e] = ((acc[e] & 0x7f7f7f7fu) + (c & 0x7f7f7f7fu)) ^ ((acc[e] ^ c) & 0x80808080u);
                }
            }
        dx[t] = uint4{acc[0], acc[1], acc[2], acc[3]};
    }
}

hipError_t maxpool_relu_grad_ws(const int8_t* x, const int8_t* y, const int8_t* dy, int n, int h, int w, int cp, int k,
                                int s, int p, int oh, int ow, int relu, int8_t* ws, int8_t* dx, hipStream_t st) {
    if (cp % 16 != 0 || k <= 0 || k > 11 || s <= 0 || ws == nullptr) return hipErrorInvalidValue;
    const int64_t tw = (int64_t)n * oh * ow * (cp / 16), tx = (int64_t)n * h * w * (cp / 16);
    if (tx >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    auto blocks = [](int64_t t) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((t + 255) / 256, 8192)); };
    hipLaunchKernelGGL(maxpool_argmax_kernel, dim3(blocks(tw)), dim3(256), 0, st, x, y, n, h, w, cp, k, s, p, oh, ow, ws);
    hipLaunchKernelGGL(maxpool_grad_gather_kernel, dim3(blocks(tx)), dim3(256), 0, st, x, ws, dy, n, h, w, cp, k, s, p,
                       oh, ow, relu, dx, (const int8_t*)nullptr);
    return hipGetLastError();
}

// the same gradient from the first-max positions the forward maxpool_nhwc16 wrote (`arg`): one pass
hipError_t maxpool_relu_grad_arg(const int8_t* x, const int8_t* arg, const int8_t* dy, int n, int h, int w, int cp,
                                 int k, int s, int p, int oh, int ow, int relu, int8_t* dx, hipStream_t st,
                                 const int8_t* pooled) {
    if (cp % 16 != 0 || k <= 0 || k > 11 || s <= 0 || arg == nullptr) return hipErrorInvalidValue;
    if (relu && pooled == nullptr && x == nullptr) return hipErrorInvalidValue;
    const int64_t tx = (int64_t)n * h * w * (cp / 16);
    if (tx >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    if (relu && pooled != nullptr && k == 3 && s == 2 && p == 1 && oh == (h - 1) / 2 + 1 && ow == (w - 1) / 2 + 1) {
        PoolGradGeom g;
        g.fg = make_fastdiv((uint32_t)(cp / 16));
        g.fw = make_fastdiv((uint32_t)w);
        g.fh = make_fastdiv((uint32_t)h);
        g.oh = oh;
        g.ow = ow;
        g.total = (uint32_t)tx;
        const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((tx + 255) / 256, 8192));
        hipLaunchKernelGGL(maxpool3_grad_pooled_kernel, dim3(blocks), dim3(256), 0, st, (const uint4*)arg,
                           (const uint4*)dy, (const uint4*)pooled, g, (uint4*)dx);
        return hipGetLastError();
    }
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((tx + 255) / 256, 8192));
    hipLaunchKernelGGL(maxpool_grad_gather_kernel, dim3(blocks), dim3(256), 0, st, x, arg, dy, n, h, w, cp, k, s, p, oh,
                       ow, relu, dx, pooled);
    return hipGetLastError();
}

__global__ void relu_grad_kernel(const int8_t* __restrict__ x, const int8_t* __restrict__ dy, int64_t n16,
                                 int64_t n, int8_t* __restrict__ out) {
    const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
        const v16c xv = ((const v16c*)x)[i];
        const v16c dv = ((const v16c*)dy)[i];
        v16c o;
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = xv[j] > 0 ? dv[j] : (signed char)0;
        ((v16c*)out)[i] = o;
    }
    const int64_t e = n16 * 16 + t0;  // the last n % 16 elements
    if (e < n) out[e] = x[e] > 0 ? dy[e] : (int8_t)0;
}

hipError_t relu_grad_nhwc16(const int8_t* x, const int8_t* dy, int64_t n, int8_t* out, hipStream_t st) {
    if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)out) & 15) return hipErrorInvalidValue;  // 16-byte vectors
    const int64_t n16 = n / 16;
    int64_t blocks = (n16 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(relu_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, dy, n16, n, out);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) loss_grad_kernel(const int8_t* __restrict__ logits, int batch, int classes,
                                                        int ld, const int8_t* __restrict__ ascale_p,
                                                        const int32_t* __restrict__ labels, int8_t* __restrict__ out) {
    loss_rows16(logits, batch, classes, ld, ascale_p, labels, out, blockIdx.x * blockDim.x + threadIdx.x);
}
// The loss gradient and the backward pass's P16 copies of the layer inputs in one launch: the
// first lw workgroups take the loss rows, the rest the conversion jobs (independent data: the
// copies read forward activations only).  Saves a launch at the head of the backward pass.
__global__ void __launch_bounds__(256) loss_grad_p16_kernel(const int8_t* __restrict__ logits, int batch, int classes,
                                                            int ld, const int8_t* __restrict__ ascale_p,
                                                            const int32_t* __restrict__ labels,
                                                            int8_t* __restrict__ out, int lw, P16Jobs J) {
    __shared__ __attribute__((aligned(16))) int8_t tile[16 * 1024];
    if ((int)blockIdx.x < lw)
        loss_rows16(logits, batch, classes, ld, ascale_p, labels, out, blockIdx.x * blockDim.x + threadIdx.x);
    else
        p16_convert_block(J, blockIdx.x - lw, tile);
}

// Exponent of a requantised weight gradient, for the DSP op slots whose graph carries one:
// the applied PSTO shift bw - rule (0 when the gradient is all zero), as the DSP ops add their
// requantisation shift to exp_in + wscale (NITI_DSPTransposeGradientConv_Int8.cpp:438-439).
__global__ void grad_exponent_kernel(const uint32_t* __restrict__ amax, int rule, int8_t* __restrict__ out) {
    const int bw = bitwidth_of(read_max(amax));  // whole wave active
    if (threadIdx.x == 0) *out = (int8_t)(bw == 0 ? 0 : bw - rule);
}
hipError_t grad_exponent(const uint32_t* amax, int rule, int8_t* out, hipStream_t st) {
    hipLaunchKernelGGL(grad_exponent_kernel, dim3(1), dim3(64), 0, st, amax, rule, out);
    return hipGetLastError();
}

// The same arithmetic for wide class rows (ImageNet heads, up to LOSS_WIDE_MAXC classes): one
// 256-thread block per sample, the row's max / sums reduced in LDS (int64, exact).
constexpr int LOSS_WIDE_PER = 8;
constexpr int LOSS_WIDE_MAXC = 256 * LOSS_WIDE_PER;
__device__ int64_t block_reduce_i64(int64_t v, bool is_max, int64_t* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = is_max ? (red[tid] > red[tid + o] ? red[tid] : red[tid + o]) : red[tid] + red[tid + o];
        __syncthreads();
    }
    const int64_t r = red[0];
    __syncthreads();
    return r;
}
__global__ void __launch_bounds__(256) loss_grad_wide_kernel(const int8_t* __restrict__ logits, int classes, int ld,
                                                             const int8_t* __restrict__ ascale_p,
                                                             const int32_t* __restrict__ labels,
                                                             int8_t* __restrict__ out) {
    __shared__ int64_t red[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int as = (int)*ascale_p;
    const int8_t* L = logits + (int64_t)i * ld;
    int64_t o[LOSS_WIDE_PER];
    if (as > -7) {
        int64_t sv[LOSS_WIDE_PER];
        int64_t mx = INT64_MIN;
#pragma unroll
        for (int k = 0; k < LOSS_WIDE_PER; ++k) {
            const int j = tid + 256 * k;
            if (j < classes) {
                int64_t t = (int64_t)L[j] * 47274;
                t = t / (1 << 15);
                sv[k] = as >= 0 ? t * ipow2_64(as) : t / ipow2_64(-as);
                mx = mx > sv[k] ? mx : sv[k];
            }
        }
        mx = block_reduce_i64(mx, true, red) - 10;
#pragma unroll
        for (int k = 0; k < LOSS_WIDE_PER; ++k) {
            const int j = tid + 256 * k;
            int64_t t = j < classes ? sv[k] - mx : 0;
            t = t > 0 ? t : 0;
            o[k] = j < classes ? ipow2_64(t) - 1 : 0;
        }
    } else {
        const int64_t base = ipow2_64(1 - 2 * (int64_t)as);
        const int64_t sb = ipow2_64(1 - (int64_t)as);
#pragma unroll
        for (int k = 0; k < LOSS_WIDE_PER; ++k) {
            const int j = tid + 256 * k;
            const int64_t t = j < classes ? L[j] : 0;
            o[k] = j < classes ? base + t * sb + t * t : 0;
        }
    }
    int64_t part = 0;
#pragma unroll
    for (int k = 0; k < LOSS_WIDE_PER; ++k) part += o[k];
    const int64_t sum = block_reduce_i64(part, false, red);
    part = 0;
#pragma unroll
    for (int k = 0; k < LOSS_WIDE_PER; ++k) {
        const int j = tid + 256 * k;
        o[k] = j < classes ? (o[k] * (1 << 11)) / sum : 0;
        part += o[k];
    }
    const int64_t gs = block_reduce_i64(part, false, red);
    const int tgt = labels[i];
    int8_t* O = out + (int64_t)i * ld;
    for (int j = tid; j < ld; j += 256) {
        const int k = j >> 8;
        int32_t gf = 0;
#pragma unroll
        for (int q = 0; q < LOSS_WIDE_PER; ++q)
            if (q == k) gf = (int32_t)(j == tgt ? o[q] - gs : o[q]);
        O[j] = j < classes ? (int8_t)psto_any(gf, 4) : (int8_t)0;
    }
}

hipError_t p16_jobs_build(const P16Conv* jobs, int n, hipStream_t st, P16Jobs* out, uint32_t* wgs_out);

hipError_t loss_grad_p16(const int8_t* logits, int batch, int classes, int ld, const int8_t* ascale,
                         const int32_t* labels, int8_t* out, const P16Conv* jobs, int n, hipStream_t st) {
    if (classes > LOSS_MAXC || ld > LOSS_WIDE_MAXC || classes > ld) {
        hipError_t e = loss_grad(logits, batch, classes, ld, ascale, labels, out, st);
        return e != hipSuccess ? e : nhwc16_to_p16_many(jobs, n, st);
    }
    P16Jobs J;
    uint32_t wg = 0;
    hipError_t e = p16_jobs_build(jobs, n, st, &J, &wg);
    if (e != hipSuccess) return e;
    const int lw = (batch + 15) / 16;
    if (J.n == 0) wg = 0;
    hipLaunchKernelGGL(loss_grad_p16_kernel, dim3((unsigned)lw + wg), dim3(256), 0, st, logits, batch, classes, ld,
                       ascale, labels, out, lw, J);
    return hipGetLastError();
}

hipError_t loss_grad(const int8_t* logits, int batch, int classes, int ld, const int8_t* ascale, const int32_t* labels,
                     int8_t* out, hipStream_t st) {
    if (classes > ld || classes > LOSS_WIDE_MAXC || ld > LOSS_WIDE_MAXC) return hipErrorInvalidValue;
    if (classes > LOSS_MAXC) {
        hipLaunchKernelGGL(loss_grad_wide_kernel, dim3((unsigned)batch), dim3(256), 0, st, logits, classes, ld, ascale,
                           labels, out);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(loss_grad_kernel, dim3((batch + 15) / 16), dim3(256), 0, st, logits, batch, classes, ld, ascale,
                       labels, out);
    return hipGetLastError();
}

// =====================================================================================
// Layout transforms
// =====================================================================================

// NHWC16 -> CHWN16 through an LDS tile: block = (pixel, 64 images, 64 channels).
__global__ void nhwc16_to_chwn16_kernel(const int8_t* __restrict__ in, int n, int hw, int cp, int np,
                                        int8_t* __restrict__ out) {
    __shared__ int8_t tile[64][64 + 4];
    const int pix = blockIdx.x;
    const int n0 = blockIdx.y * 64, c0 = blockIdx.z * 64;
    const int t = threadIdx.x;
    {   // read: row = image, 4 x 16B chunks of channels
        const int r = t >> 2, ch = (t & 3) * 16;
        v16c v;
        if (n0 + r < n && c0 + ch < cp)
            v = *(const v16c*)(in + ((int64_t)(n0 + r) * hw + pix) * cp + c0 + ch);
        else
            for (int j = 0; j < 16; ++j) v[j] = 0;
        for (int j = 0; j < 16; ++j) tile[r][ch + j] = v[j];
    }
    __syncthreads();
    {   // write: row = channel, 4 x 16B chunks of images
        const int c = t >> 2, nb = (t & 3) * 16;
        if (c0 + c < cp && n0 + nb < np) {
            v16c v;
            for (int j = 0; j < 16; ++j) v[j] = tile[nb + j][c];
            *(v16c*)(out + ((int64_t)(c0 + c) * hw + pix) * np + n0 + nb) = v;
        }
    }
}

hipError_t nhwc16_to_chwn16(const int8_t* in, int n, int hw, int cp, int np, int8_t* out, hipStream_t st) {
    dim3 grid(hw, (np + 63) / 64, (cp + 63) / 64);
    hipLaunchKernelGGL(nhwc16_to_chwn16_kernel, grid, dim3(256), 0, st, in, n, hw, cp, np, out);
    return hipGetLastError();
}

struct OhwiToIhwo {
    const int8_t* w;
    int co, ci, kk, cip, cop;
    int8_t* wt;
    __device__ void operator()(int64_t i) const {  // i over [ci][kk][cop]
        const int o = (int)(i % cop);
        const int64_t r = i / cop;
        const int k = (int)(r % kk);
        const int c = (int)(r / kk);
        wt[i] = o < co ? w[((int64_t)o * kk + k) * cip + c] : (int8_t)0;
    }
};
hipError_t ohwi16_to_ihwo16(const int8_t* w, int co, int ci, int kk, int cip, int cop, int8_t* wt, hipStream_t st) {
    return launch_map((int64_t)ci * kk * cop, OhwiToIhwo{w, co, ci, kk, cip, cop, wt}, st);
}

struct C4ToNhwc16 {
    const int8_t* x;
    int n, c, hw, cp;
    int8_t* out;
    __device__ void operator()(int64_t i) const {  // i over [n][hw][cp]
        const int ch = (int)(i % cp);
        const int64_t r = i / cp;
        const int64_t p = r % hw;
        const int64_t b = r / hw;
        out[i] = ch < c ? x[(((int64_t)(ch >> 2) * n + b) * hw + p) * 4 + (ch & 3)] : (int8_t)0;
    }
};
hipError_t c4_to_nhwc16(const int8_t* x, int n, int c, int hw, int cp, int8_t* out, hipStream_t st) {
    return launch_map((int64_t)n * hw * cp, C4ToNhwc16{x, n, c, hw, cp, out}, st);
}

struct NchwToNhwc16 {
    const int8_t* x;
    int n, c, hw, cp;
    int8_t* out;
    __device__ void operator()(int64_t i) const {
        const int ch = (int)(i % cp);
        const int64_t r = i / cp;
        const int64_t p = r % hw;
        const int64_t b = r / hw;
        out[i] = ch < c ? x[((int64_t)b * c + ch) * hw + p] : (int8_t)0;
    }
};
hipError_t nchw_to_nhwc16(const int8_t* x, int n, int c, int hw, int cp, int8_t* out, hipStream_t st) {
    return launch_map((int64_t)n * hw * cp, NchwToNhwc16{x, n, c, hw, cp, out}, st);
}

struct NchwToChwn16 {
    const int8_t* x;
    int n, c, hw, cp, np;
    int8_t* out;
    __device__ void operator()(int64_t i) const {  // i over [cp][hw][np]
        const int b = (int)(i % np);
        const int64_t r = i / np;
        const int64_t p = r % hw;
        const int ch = (int)(r / hw);
        out[i] = (ch < c && b < n) ? x[((int64_t)b * c + ch) * hw + p] : (int8_t)0;
    }
};
hipError_t nchw_to_chwn16(const int8_t* x, int n, int c, int hw, int cp, int np, int8_t* out, hipStream_t st) {
    return launch_map((int64_t)cp * hw * np, NchwToChwn16{x, n, c, hw, cp, np, out}, st);
}

struct C4ToChwn16 {
    const int8_t* x;
    int n, c, hw, cp, np;
    int8_t* out;
    __device__ void operator()(int64_t i) const {
        const int b = (int)(i % np);
        const int64_t r = i / np;
        const int64_t p = r % hw;
        const int ch = (int)(r / hw);
        out[i] = (ch < c && b < n) ? x[(((int64_t)(ch >> 2) * n + b) * hw + p) * 4 + (ch & 3)] : (int8_t)0;
    }
};
hipError_t c4_to_chwn16(const int8_t* x, int n, int c, int hw, int cp, int np, int8_t* out, hipStream_t st) {
    return launch_map((int64_t)cp * hw * np, C4ToChwn16{x, n, c, hw, cp, np, out}, st);
}

struct Nhwc16ToNchw {
    const int8_t* x;
    int n, c, hw, cp;
    int8_t* out;
    __device__ void operator()(int64_t i) const {  // i over [n][c][hw]
        const int64_t p = i % hw;
        const int64_t r = i / hw;
        const int ch = (int)(r % c);
        const int64_t b = r / c;
        out[i] = x[(b * hw + p) * cp + ch];
    }
};
hipError_t nhwc16_to_nchw(const int8_t* x, int n, int c, int hw, int cp, int8_t* out, hipStream_t st) {
    return launch_map((int64_t)n * c * hw, Nhwc16ToNchw{x, n, c, hw, cp, out}, st);
}

struct OihwToOhwi16 {
    const int8_t* w;
    int co, ci, kk, cip, rev;
    int8_t* out;
    __device__ void operator()(int64_t i) const {  // i over [co][kk][cip]
        const int c = (int)(i % cip);
        const int64_t r = i / cip;
        const int k = (int)(r % kk);
        const int64_t o = r / kk;
        const int ks = rev ? kk - 1 - k : k;  // rotate180 == reversing the KH*KW plane
        out[i] = c < ci ? w[(o * ci + c) * kk + ks] : (int8_t)0;
    }
};
hipError_t oihw_to_ohwi16(const int8_t* w, int co, int ci, int kk, int cip, int8_t* out, hipStream_t st,
                          bool reverse_taps) {
    return launch_map((int64_t)co * kk * cip, OihwToOhwi16{w, co, ci, kk, cip, reverse_taps ? 1 : 0, out}, st);
}

struct OihwToIhwo16 {
    const int8_t* w;
    int co, ci, kk, cop;
    int8_t* out;
    __device__ void operator()(int64_t i) const {  // i over [ci][kk][cop]
        const int o = (int)(i % cop);
        const int64_t r = i / cop;
        const int k = (int)(r % kk);
        const int64_t c = r / kk;
        out[i] = o < co ? w[((int64_t)o * ci + c) * kk + k] : (int8_t)0;
    }
};
hipError_t oihw_to_ihwo16(const int8_t* w, int co, int ci, int kk, int cop, int8_t* out, hipStream_t st) {
    return launch_map((int64_t)ci * kk * cop, OihwToIhwo16{w, co, ci, kk, cop, out}, st);
}

struct Ohwi16ToOihw {
    const int8_t* w;
    int co, ci, kk, cip;
    int8_t* out;
    __device__ void operator()(int64_t i) const {  // i over [co][ci][kk]
        const int k = (int)(i % kk);
        const int64_t r = i / kk;
        const int c = (int)(r % ci);
        const int64_t o = r / ci;
        out[i] = w[(o * kk + k) * cip + c];
    }
};
hipError_t ohwi16_to_oihw(const int8_t* w, int co, int ci, int kk, int cip, int8_t* out, hipStream_t st) {
    return launch_map((int64_t)co * ci * kk, Ohwi16ToOihw{w, co, ci, kk, cip, out}, st);
}

struct PadRows {
    const int8_t* in;
    int rows, cols, ld;
    int8_t* out;
    __device__ void operator()(int64_t i) const {
        const int c = (int)(i % ld);
        const int64_t r = i / ld;
        out[i] = c < cols ? in[r * cols + c] : (int8_t)0;
    }
};
hipError_t pad_rows(const int8_t* in, int rows, int cols, int ld, int8_t* out, hipStream_t st) {
    return launch_map((int64_t)rows * ld, PadRows{in, rows, cols, ld, out}, st);
}

struct TransposeI32 {
    const int32_t* in;
    int rows, cols, ld;
    int32_t* out;
    __device__ void operator()(int64_t i) const {  // out [cols][rows]
        const int r = (int)(i % rows);
        const int64_t c = i / rows;
        out[i] = in[(int64_t)r * ld + c];
    }
};
hipError_t transpose_i32(const int32_t* in, int rows, int cols, int ld, int32_t* out, hipStream_t st) {
    return launch_map((int64_t)rows * cols, TransposeI32{in, rows, cols, ld, out}, st);
}

}  // namespace niti
