// niti_depthwise.hip -- depthwise conv layers (dwconv_*, niti_kernels.hpp): c_out == c_in == C, a
// square 3x3 or 5x5 kernel, stride 1 or 2 (S, both ways), one pad on every side.
//
// The layer is NITI_Conv_Int8 over the block-diagonal dense weight W[o][i] = (o == i) ? w[o] : 0, so
// there is no contraction over input channels and no MFMA shape fits: the three launches are plain
// VALU kernels; measured, their multiply-adds and not memory bound them.
//
// Layouts.  Activations NHWC16 [n][h][w][cp].  The weight, its int32 gradient and the gradient's
// partial slabs are [k * k][cp], tap-major: the dense OHWI16 form of a c_out = 1, c_in = C layer, so
// the update launch, its combine and splitk_reduce_linear take them as they stand.
//
// dwconv_act (forward at either stride and the stride-1 input gradient: that is the same conv on dy
// with the taps reversed and pad k - 1 - pad; the stride-2 input gradient is dwconv_dgrad2 below).
// A lane owns one output column and 16 channels and walks DW_ROWS output rows down; per output it loads its k * k taps, 16 bytes each, and recomputes the 16
// accumulators in both passes: no int32 tensor is written.  Neighbouring outputs share taps through
// the caches (a workgroup's lanes are adjacent columns of a row band), so HBM sees each input byte
// once, up to a band's halo rows.  A tap
// outside the image is a load at offset OOB, decided from its row and column, never by where the
// address happens to fall.  Pass 0 publishes max|acc|, pass 1 reads the range (after any MAX
// all-reduce) and requantises by NITI_Conv_Int8.cpp:260-307's rule, chosen once per wave.
//
// dwconv_wgrad.  A lane owns 16 channels and one tap row ky and walks output rows along x with a
// window of k input pixels: k x 16 accumulators in registers, two loads per step (issued one step
// ahead).  The lanes of a workgroup that share (channels, ky) sum through LDS and the workgroup
// writes its part of one slab; the slab count is a function of the shape alone.
#include <algorithm>

#include "niti_device.hpp"
#include "niti_kernels.hpp"
#include "niti_sgd.hpp"

namespace niti {

namespace {

constexpr int DW_ROWS = 8;          // output rows a lane of dwconv_act walks
constexpr int DW_WG_GROUPS = 16;    // channel groups (of 16) per weight-gradient workgroup, at most
constexpr int DW_MAX_SLABS = 1024;
constexpr size_t DW_SLAB_BYTES = size_t(4) << 20;  // of all slabs, past 64 of them: the combine reads every one

// byte e of dword a times byte e of dword b, both signed
__device__ __forceinline__ int bmul(int a, int b, int e) {
    return (int)(int8_t)((uint32_t)a >> (8 * e)) * (int)(int8_t)((uint32_t)b >> (8 * e));
}

struct DwActArgs {
    const int8_t* x;  // [n][ih][iw][cp]
    const int8_t* w;  // [k * k][cp]
    int8_t* out;      // [n][oh][ow][cp]
    const int8_t* relu_mask;
    uint32_t xbytes, wbytes, obytes;
    int ih, iw, oh, ow, cp, pad, flip, relu;
    int cols;    // ow * cp / 16
    int units;   // cols * bands per image * n: one lane each
    FastDiv fcols, fbands, fg;  // by columns, bands per image, channel groups
    uint32_t* amax;
    const int8_t* exp_in;
    const int8_t* wscale;
    int8_t* exp_out;
};

// 4 x 4 byte transpose: R[e] = bytes e of (A, B, C, D), A's lowest
__device__ __forceinline__ void tr4(int A, int B, int C, int D, int (&R)[4]) {
    const uint32_t ab_lo = __builtin_amdgcn_perm((uint32_t)B, (uint32_t)A, 0x05010400u);
    const uint32_t ab_hi = __builtin_amdgcn_perm((uint32_t)B, (uint32_t)A, 0x07030602u);
    const uint32_t cd_lo = __builtin_amdgcn_perm((uint32_t)D, (uint32_t)C, 0x05010400u);
    const uint32_t cd_hi = __builtin_amdgcn_perm((uint32_t)D, (uint32_t)C, 0x07030602u);
    R[0] = (int)__builtin_amdgcn_perm(cd_lo, ab_lo, 0x05040100u);
    R[1] = (int)__builtin_amdgcn_perm(cd_lo, ab_lo, 0x07060302u);
    R[2] = (int)__builtin_amdgcn_perm(cd_hi, ab_hi, 0x05040100u);
    R[3] = (int)__builtin_amdgcn_perm(cd_hi, ab_hi, 0x07060302u);
}

// The multiply-adds run on v_dot4c_i32_i8: four taps' pixels (one dword = 4 channels each) are
// transposed into one dword per channel (8 v_perm_b32) and meet the weights, packed the same way once
// per lane: 12 instructions per 16 multiply-adds, against about 2.5 per multiply-add for byte
// extracts and v_mad.  k * k = 4 NG + 1: the last tap goes the plain way.
template <int K, int PASS, int S>
__global__ void __launch_bounds__(256) dwconv_act_kernel(DwActArgs a) {
    constexpr int KK = K * K, NG = KK / 4;
    static_assert(KK % 4 == 1, "four taps per dot, one left over");
    const int lane = threadIdx.x & 63;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.xbytes), rw = make_rsrc(a.w, a.wbytes);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(a.out, PASS == 1 ? a.obytes : 0u);
    const __amdgpu_buffer_rsrc_t rm = make_rsrc(a.relu_mask, PASS == 1 && a.relu_mask != nullptr ? a.obytes : 0u);
    uint32_t gm = 0;
    if (PASS == 1) gm = a.amax[lane * MAX_SLOT_STRIDE];

    // lane = (image, row band, column, channel group), channel groups fastest: a narrow map's workgroup
    // spans several bands and no lane idles
    const uint32_t unit = blockIdx.x * 256u + threadIdx.x;
    const bool active = unit < (uint32_t)a.units;
    const uint32_t band = fdiv(a.fcols, unit), col = unit - band * a.fcols.d;
    const uint32_t img = fdiv(a.fbands, band), rb = band - img * a.fbands.d;
    const uint32_t ox = fdiv(a.fg, col), cg = col - ox * a.fg.d;
    const int oy0 = (int)rb * DW_ROWS;
    const int oy1 = active ? min(oy0 + DW_ROWS, a.oh) : oy0;

    // this lane's weights: wp[g][4 j + e] = taps 4 g .. 4 g + 3 of channel 4 j + e; wl the last tap
    auto wload = [&](int t) {
        return buf_load16(rw, active ? (uint32_t)((a.flip ? KK - 1 - t : t) * a.cp) + cg * 16u : OOB);
    };
    int wp[NG][16];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const v4i w0 = wload(4 * g), w1 = wload(4 * g + 1), w2 = wload(4 * g + 2), w3 = wload(4 * g + 3);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int R[4];
            tr4(w0[j], w1[j], w2[j], w3[j], R);
#pragma unroll
            for (int e = 0; e < 4; ++e) wp[g][4 * j + e] = R[e];
        }
    }
    const v4i wl = wload(KK - 1);

    int s = 2;
    bool raw = true;
    if (PASS == 1) {
        const int shift = __builtin_amdgcn_readfirstlane(bitwidth_of(wave_max(gm))) - 7;
        s = shift > 1 ? shift : 2;
        raw = shift <= 0;
        if (blockIdx.x == 0 && threadIdx.x == 0 && a.exp_out != nullptr) {
            const int inc = shift > 1 ? shift : (shift == 1 ? 2 : 0);
            *a.exp_out = (int8_t)((a.exp_in ? (int)*a.exp_in : 0) + (a.wscale ? (int)*a.wscale : 0) + inc);
        }
    }

    uint32_t m = 0;
    for (int oy = oy0; oy < oy1; ++oy) {
        // tap t of this output: input pixel (S oy - pad + t / K, S ox - pad + t % K); outside the image: zeros
        auto xload = [&](int t) {
            const int iy = S * oy - a.pad + t / K, ix = S * (int)ox - a.pad + t % K;
            const bool ok = active && iy >= 0 && iy < a.ih && ix >= 0 && ix < a.iw;
            return buf_load16(
                rx, ok ? ((img * (uint32_t)a.ih + (uint32_t)iy) * (uint32_t)a.iw + (uint32_t)ix) * (uint32_t)a.cp + cg * 16u
                       : OOB);
        };
        int acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const v4i p0 = xload(4 * g), p1 = xload(4 * g + 1), p2 = xload(4 * g + 2), p3 = xload(4 * g + 3);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int R[4];
                tr4(p0[j], p1[j], p2[j], p3[j], R);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * j + e] = __builtin_amdgcn_sdot4(R[e], wp[g][4 * j + e], acc[4 * j + e], false);
            }
        }
        {
            const v4i p = xload(KK - 1);
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] += bmul(p[j >> 2], wl[j >> 2], j & 3);
        }
        if (PASS == 0) {
#pragma unroll
            for (int j = 0; j < 16; ++j) m = max(m, uabs32(acc[j]));
        } else {
            const uint32_t off =
                active ? ((img * (uint32_t)a.oh + (uint32_t)oy) * (uint32_t)a.ow + ox) * (uint32_t)a.cp + cg * 16u : OOB;
            v4i mk{0, 0, 0, 0};
            if (a.relu_mask != nullptr) mk = buf_load16(rm, off);
            v4i q;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t o = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int32_t v = raw ? (int32_t)(int8_t)acc[4 * d + e] : psto_fast(acc[4 * d + e], s);
                    if (a.relu && v < 0) v = 0;
                    if (a.relu_mask != nullptr && (int8_t)((uint32_t)mk[d] >> (8 * e)) <= 0) v = 0;
                    o |= ((uint32_t)v & 0xffu) << (8 * e);
                }
                q[d] = (int)o;
            }
            buf_store16(ro, off, q);
        }
    }

    if (PASS == 0) {
        m = wave_max(m);
        __shared__ uint32_t red[4];
        if (lane == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) publish_max(a.amax, max(max(red[0], red[1]), max(red[2], red[3])));
    }
}

// The stride-2 input gradient, by pixel parity.  dx(y, x) sums dy((y + pad - ky) / 2, (x + pad - kx) / 2) w(ky, kx)
// over the taps with both numerators even: the pixels of one parity class (y & 1, x & 1) share one tap subset,
// ky = ky0, ky0 + 2, .. with ky0 = (y + pad) & 1 (and so for kx).  blockIdx.y is the class, so a wave holds one
// class and runs its taps alone (4 / 2 / 2 / 1 of 9, 9 / 6 / 6 / 4 of 25): dy is read where it lies, there is no
// zero-stuffed copy.  A lane owns one class column and 16 channels and walks DW_ROWS class rows down.  Pixels
// no output reads have every tap outside dy: they are written as zeros like any other.
struct DwDg2Args {
    const int8_t* dy;  // [n][oh][ow][cp]
    const int8_t* w;   // [k * k][cp]
    int8_t* out;       // [n][h][w][cp]
    const int8_t* relu_mask;
    uint32_t dbytes, wbytes, obytes;
    int h, w_, oh, ow, cp, pad;
    int units[4];                // lanes of class 2 (y & 1) + (x & 1)
    FastDiv fcols[4], fbands[4];  // by the class's columns x channel groups, its bands per image
    FastDiv fg;
    uint32_t* amax;
    const int8_t* exp_in;
    const int8_t* wscale;
    int8_t* exp_out;
};

template <int K, int PASS, int KY0, int KX0>
__device__ __forceinline__ void dw_dgrad2_class(const DwDg2Args& a, int cls, uint32_t gm) {
    constexpr int NY = KY0 ? K / 2 : (K + 1) / 2, NX = KX0 ? K / 2 : (K + 1) / 2;
    constexpr int NT = NY * NX, REM = NT % 4;
    constexpr int NG = NT / 4 + (REM >= 2 ? 1 : 0);  // dots of four taps; a last group of 2 or 3 is zero-filled
    constexpr int NGA = NG > 0 ? NG : 1;
    const int lane = threadIdx.x & 63;
    const __amdgpu_buffer_rsrc_t rd = make_rsrc(a.dy, a.dbytes), rw = make_rsrc(a.w, a.wbytes);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(a.out, PASS == 1 ? a.obytes : 0u);
    const __amdgpu_buffer_rsrc_t rm = make_rsrc(a.relu_mask, PASS == 1 && a.relu_mask != nullptr ? a.obytes : 0u);
    const int py = cls >> 1, px = cls & 1;
    const int hy = (a.h - py + 1) >> 1;  // class rows
    // dy row of class row yi and tap row j: by + yi - j (ky = KY0 + 2 j)
    const int by = (py + a.pad - KY0) >> 1, bx = (px + a.pad - KX0) >> 1;

    const uint32_t unit = blockIdx.x * 256u + threadIdx.x;
    const bool active = unit < (uint32_t)a.units[cls];
    const uint32_t band = fdiv(a.fcols[cls], unit), col = unit - band * a.fcols[cls].d;
    const uint32_t img = fdiv(a.fbands[cls], band), rb = band - img * a.fbands[cls].d;
    const uint32_t xi = fdiv(a.fg, col), cg = col - xi * a.fg.d;
    const int yi0 = (int)rb * DW_ROWS;
    const int yi1 = active ? min(yi0 + DW_ROWS, hy) : yi0;

    auto wload = [&](int t) {
        const int tap = (KY0 + 2 * (t / NX)) * K + KX0 + 2 * (t % NX);
        return buf_load16(rw, active && t < NT ? (uint32_t)(tap * a.cp) + cg * 16u : OOB);
    };
    int wp[NGA][16];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const v4i w0 = wload(4 * g), w1 = wload(4 * g + 1), w2 = wload(4 * g + 2), w3 = wload(4 * g + 3);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int R[4];
            tr4(w0[j], w1[j], w2[j], w3[j], R);
#pragma unroll
            for (int e = 0; e < 4; ++e) wp[g][4 * j + e] = R[e];
        }
    }
    const v4i wl = wload(REM == 1 ? NT - 1 : NT);

    int s = 2;
    bool raw = true;
    if (PASS == 1) {
        const int shift = __builtin_amdgcn_readfirstlane(bitwidth_of(wave_max(gm))) - 7;
        s = shift > 1 ? shift : 2;
        raw = shift <= 0;
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && a.exp_out != nullptr) {
            const int inc = shift > 1 ? shift : (shift == 1 ? 2 : 0);
            *a.exp_out = (int8_t)((a.exp_in ? (int)*a.exp_in : 0) + (a.wscale ? (int)*a.wscale : 0) + inc);
        }
    }

    uint32_t m = 0;
    for (int yi = yi0; yi < yi1; ++yi) {
        // tap t of this pixel: dy pixel (by + yi - t / NX, bx + xi - t % NX); outside dy (or past the taps): zeros
        auto dload = [&](int t) {
            const int oy = by + yi - t / NX, ox = bx + (int)xi - t % NX;
            const bool ok = active && t < NT && oy >= 0 && oy < a.oh && ox >= 0 && ox < a.ow;
            return buf_load16(
                rd, ok ? ((img * (uint32_t)a.oh + (uint32_t)oy) * (uint32_t)a.ow + (uint32_t)ox) * (uint32_t)a.cp + cg * 16u
                       : OOB);
        };
        int acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const v4i p0 = dload(4 * g), p1 = dload(4 * g + 1), p2 = dload(4 * g + 2), p3 = dload(4 * g + 3);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int R[4];
                tr4(p0[j], p1[j], p2[j], p3[j], R);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * j + e] = __builtin_amdgcn_sdot4(R[e], wp[g][4 * j + e], acc[4 * j + e], false);
            }
        }
        if (REM == 1) {
            const v4i p = dload(NT - 1);
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] += bmul(p[j >> 2], wl[j >> 2], j & 3);
        }
        if (PASS == 0) {
#pragma unroll
            for (int j = 0; j < 16; ++j) m = max(m, uabs32(acc[j]));
        } else {
            const uint32_t y = (uint32_t)(py + 2 * yi), x = (uint32_t)px + 2u * xi;
            const uint32_t off =
                active ? ((img * (uint32_t)a.h + y) * (uint32_t)a.w_ + x) * (uint32_t)a.cp + cg * 16u : OOB;
            v4i mk{0, 0, 0, 0};
            if (a.relu_mask != nullptr) mk = buf_load16(rm, off);
            v4i q;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t o = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int32_t v = raw ? (int32_t)(int8_t)acc[4 * d + e] : psto_fast(acc[4 * d + e], s);
                    if (a.relu_mask != nullptr && (int8_t)((uint32_t)mk[d] >> (8 * e)) <= 0) v = 0;
                    o |= ((uint32_t)v & 0xffu) << (8 * e);
                }
                q[d] = (int)o;
            }
            buf_store16(ro, off, q);
        }
    }

    if (PASS == 0) {
        m = wave_max(m);
        __shared__ uint32_t red[4];
        if (lane == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) publish_max(a.amax, max(max(red[0], red[1]), max(red[2], red[3])));
    }
}

template <int K, int PASS>
__global__ void __launch_bounds__(256) dwconv_dgrad2_kernel(DwDg2Args a) {
    uint32_t gm = 0;
    if (PASS == 1) gm = a.amax[(threadIdx.x & 63) * MAX_SLOT_STRIDE];
    // (uniform over the workgroup: the class is blockIdx.y)
    const int cls = (int)blockIdx.y;
    const int ky0 = ((cls >> 1) + a.pad) & 1, kx0 = ((cls & 1) + a.pad) & 1;
    if (ky0 == 0 && kx0 == 0)
        dw_dgrad2_class<K, PASS, 0, 0>(a, cls, gm);
    else if (ky0 == 0)
        dw_dgrad2_class<K, PASS, 0, 1>(a, cls, gm);
    else if (kx0 == 0)
        dw_dgrad2_class<K, PASS, 1, 0>(a, cls, gm);
    else
        dw_dgrad2_class<K, PASS, 1, 1>(a, cls, gm);
}

struct DwWgArgs {
    const int8_t* x;   // [n][h][w][cp]
    const int8_t* dy;  // [n][oh][ow][cp]
    int32_t* slab;     // [gridDim.x][k * k][cp]
    uint32_t xbytes, dbytes, sbytes;
    int h, w, oh, ow, cp, pad;
    int G, GB, R;  // channel groups; those of a workgroup; output rows a workgroup takes at once
    int rows;      // n * oh
    FastDiv fgb, foh;
};

template <int K, int S>
__global__ void __launch_bounds__(256) dwconv_wgrad_kernel(DwWgArgs a) {
    __shared__ __attribute__((aligned(16))) int32_t red[256 * 16];
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.xbytes), rd = make_rsrc(a.dy, a.dbytes);
    const uint32_t t = threadIdx.x;
    const uint32_t rest = fdiv(a.fgb, t), cgl = t - rest * (uint32_t)a.GB;
    const uint32_t r = rest / (uint32_t)K, ky = rest - r * (uint32_t)K;
    const uint32_t cg = blockIdx.y * (uint32_t)a.GB + cgl;
    const bool active = r < (uint32_t)a.R && cg < (uint32_t)a.G;
    const uint32_t cp = (uint32_t)a.cp;

    int acc[K][16];
#pragma unroll
    for (int c = 0; c < K; ++c)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[c][j] = 0;

    for (uint32_t row = blockIdx.x * (uint32_t)a.R + r; row < (uint32_t)a.rows; row += gridDim.x * (uint32_t)a.R) {
        const uint32_t img = fdiv(a.foh, row), oy = row - img * (uint32_t)a.oh;
        const int iy = S * (int)oy + (int)ky - a.pad;
        const bool rok = active && iy >= 0 && iy < a.h;  // (a tap row outside the image adds nothing)
        const uint32_t x0 = (img * (uint32_t)a.h + (uint32_t)iy) * (uint32_t)a.w;
        const uint32_t d0 = row * (uint32_t)a.ow;
        auto xload = [&](int ix) {
            return buf_load16(rx, rok && ix >= 0 && ix < a.w ? (x0 + (uint32_t)ix) * cp + cg * 16u : OOB);
        };
        auto dload = [&](int ox) {
            return buf_load16(rd, rok && ox < a.ow ? (d0 + (uint32_t)ox) * cp + cg * 16u : OOB);
        };
        // the window at step ox: input columns S ox - pad .. S ox - pad + K - 1
        v4i win[K];
#pragma unroll
        for (int c = 0; c < K; ++c) win[c] = xload(c - a.pad);
        v4i d = dload(0);
        for (int ox = 0; ox < a.ow; ++ox) {
            v4i xn[S];
#pragma unroll
            for (int e = 0; e < S; ++e) xn[e] = xload(S * ox + K - a.pad + e);
            const v4i dn = dload(ox + 1);
#pragma unroll
            for (int c = 0; c < K; ++c)
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[c][j] += bmul(d[j >> 2], win[c][j >> 2], j & 3);
#pragma unroll
            for (int c = 0; c + S < K; ++c) win[c] = win[c + S];
#pragma unroll
            for (int e = 0; e < S; ++e) win[K - S + e] = xn[e];
            d = dn;
        }
    }

    // lanes t = cgl + GB * (ky + K * r) that share (cgl, ky) sum over r through LDS, one kx at a time
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.slab, a.sbytes);
    const uint32_t combos = (uint32_t)(a.GB * K);
#pragma unroll
    for (int c = 0; c < K; ++c) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *(v4i*)(red + t * 16 + 4 * q) = v4i{acc[c][4 * q], acc[c][4 * q + 1], acc[c][4 * q + 2], acc[c][4 * q + 3]};
        __syncthreads();
        for (uint32_t e = t; e < combos * 4u; e += 256u) {
            const uint32_t combo = e >> 2, q = e & 3u;
            v4i sum{0, 0, 0, 0};
            for (int rr = 0; rr < a.R; ++rr) sum += *(const v4i*)(red + ((uint32_t)rr * combos + combo) * 16 + 4 * q);
            const uint32_t kyo = fdiv(a.fgb, combo), cgo = blockIdx.y * (uint32_t)a.GB + (combo - kyo * (uint32_t)a.GB);
            const uint32_t tap = kyo * (uint32_t)K + (uint32_t)c;
            const uint32_t off = ((blockIdx.x * (uint32_t)(K * K) + tap) * cp + cgo * 16u + q * 4u) * 4u;
            buf_store16(rs, cgo < (uint32_t)a.G ? off : OOB, sum);
        }
    }
}

struct DwWgPlan {
    int G, GB, R, gy, slabs;
};
DwWgPlan dw_wgrad_plan(const ConvGeom& g) {
    DwWgPlan p;
    p.G = g.cip / 16;
    p.GB = std::min(p.G, DW_WG_GROUPS);
    p.R = 256 / (p.GB * g.kh);
    p.gy = (p.G + p.GB - 1) / p.GB;
    const int64_t rows = (int64_t)g.n * g.oh;
    const int64_t one = (int64_t)g.kh * g.kw * g.cip * sizeof(int32_t);
    const int64_t cap = std::max<int64_t>(64, std::min<int64_t>(DW_MAX_SLABS, (int64_t)DW_SLAB_BYTES / one));
    p.slabs = (int)std::max<int64_t>(1, std::min<int64_t>(cap, (rows + p.R - 1) / p.R));
    return p;
}

// the stride-2 input gradient (the checks are dw_act's)
hipError_t dw_dgrad2(const ConvGeom& g, const int8_t* dy, const int8_t* w, uint32_t* amax, const ActOut& o, int pass,
                     hipStream_t st) {
    DwDg2Args a{};
    a.dy = dy;
    a.w = w;
    a.out = o.out;
    a.relu_mask = o.relu_mask;
    a.h = g.h;
    a.w_ = g.w;
    a.oh = g.oh;
    a.ow = g.ow;
    a.cp = g.cip;
    a.pad = g.pt;
    a.dbytes = (uint32_t)((int64_t)g.n * g.oh * g.ow * g.cip);
    a.obytes = (uint32_t)((int64_t)g.n * g.h * g.w * g.cip);
    a.wbytes = (uint32_t)(g.kh * g.kw * g.cip);
    const int G = g.cip / 16;
    int64_t most = 1;
    for (int cls = 0; cls < 4; ++cls) {
        const int hy = (g.h - (cls >> 1) + 1) / 2, wx = (g.w - (cls & 1) + 1) / 2;
        const int bands = (hy + DW_ROWS - 1) / DW_ROWS;
        const int64_t units = (int64_t)wx * G * bands * g.n;
        if (units > 0x7fffffff) return hipErrorInvalidValue;
        a.units[cls] = (int)units;
        a.fcols[cls] = make_fastdiv((uint32_t)std::max(1, wx * G));
        a.fbands[cls] = make_fastdiv((uint32_t)std::max(1, bands));
        most = std::max(most, units);
    }
    a.fg = make_fastdiv((uint32_t)G);
    a.amax = amax;
    a.exp_in = o.exp_in;
    a.wscale = o.wscale;
    a.exp_out = o.exp_out;
    using Kern = void (*)(DwDg2Args);
    const Kern f = g.kh == 3 ? (pass == 0 ? dwconv_dgrad2_kernel<3, 0> : dwconv_dgrad2_kernel<3, 1>)
                             : (pass == 0 ? dwconv_dgrad2_kernel<5, 0> : dwconv_dgrad2_kernel<5, 1>);
    hipLaunchKernelGGL(f, dim3((unsigned)((most + 255) / 256), 4), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t dw_act(const ConvGeom& g, bool dgrad, const int8_t* in, const int8_t* w, uint32_t* amax, const ActOut& o,
                  int pass, hipStream_t st) {
    if (!dwconv2_ok(g) || in == nullptr || w == nullptr || amax == nullptr || pass < 0 || pass > 1)
        return hipErrorInvalidValue;
    // the fields this launch honours: out, relu (forward), relu_mask (input gradient), the exponents
    if (o.pool.pool_out != nullptr || o.pool.x != nullptr || o.pool.y != nullptr || o.pool.dx != nullptr ||
        o.pool.dx_c32 != nullptr || o.out_p16 != nullptr || o.zero_cls != 0 || o.pool3.out != nullptr ||
        o.pool3.arg != nullptr)
        return hipErrorInvalidValue;
    if ((dgrad && o.relu != 0) || (!dgrad && o.relu_mask != nullptr)) return hipErrorInvalidValue;
    if (pass == 1 && o.out == nullptr) return hipErrorInvalidValue;
    if (dgrad && g.sh == 2) return dw_dgrad2(g, in, w, amax, o, pass, st);
    DwActArgs a{};
    a.x = in;
    a.w = w;
    a.out = o.out;
    a.relu_mask = o.relu_mask;
    a.cp = g.cip;
    a.ih = dgrad ? g.oh : g.h;
    a.iw = dgrad ? g.ow : g.w;
    a.oh = dgrad ? g.h : g.oh;
    a.ow = dgrad ? g.w : g.ow;
    a.pad = dgrad ? g.kh - 1 - g.pt : g.pt;
    a.flip = dgrad ? 1 : 0;
    a.relu = o.relu;
    a.xbytes = (uint32_t)((int64_t)g.n * a.ih * a.iw * a.cp);
    a.obytes = (uint32_t)((int64_t)g.n * a.oh * a.ow * a.cp);
    a.wbytes = (uint32_t)(g.kh * g.kw * a.cp);
    a.cols = a.ow * (a.cp / 16);
    const int bands = (a.oh + DW_ROWS - 1) / DW_ROWS;
    const int64_t units = (int64_t)a.cols * bands * g.n;
    if (units > 0x7fffffff) return hipErrorInvalidValue;
    a.units = (int)units;
    a.fcols = make_fastdiv((uint32_t)a.cols);
    a.fbands = make_fastdiv((uint32_t)bands);
    a.fg = make_fastdiv((uint32_t)(a.cp / 16));
    a.amax = amax;
    a.exp_in = o.exp_in;
    a.wscale = o.wscale;
    a.exp_out = o.exp_out;
    const int64_t grid = (units + 255) / 256;
    using Kern = void (*)(DwActArgs);
    const Kern f1 = g.kh == 3 ? (pass == 0 ? dwconv_act_kernel<3, 0, 1> : dwconv_act_kernel<3, 1, 1>)
                              : (pass == 0 ? dwconv_act_kernel<5, 0, 1> : dwconv_act_kernel<5, 1, 1>);
    const Kern f2 = g.kh == 3 ? (pass == 0 ? dwconv_act_kernel<3, 0, 2> : dwconv_act_kernel<3, 1, 2>)
                              : (pass == 0 ? dwconv_act_kernel<5, 0, 2> : dwconv_act_kernel<5, 1, 2>);
    const Kern f = g.sh == 2 ? f2 : f1;
    hipLaunchKernelGGL(f, dim3((unsigned)grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace

bool dwconv_ok(const ConvGeom& g) { return g.sh == 1 && g.sw == 1 && dwconv2_ok(g); }

bool dwconv2_ok(const ConvGeom& g) {
    if (g.n < 1 || g.c_in < 1 || g.c_in != g.c_out || g.kh != g.kw || (g.kh != 3 && g.kh != 5)) return false;
    if ((g.sh != 1 && g.sh != 2) || g.sw != g.sh || g.dh != 1 || g.dw != 1) return false;
    if (g.pt < 0 || g.pt >= g.kh || g.pl != g.pt || g.pb != g.pt || g.pr != g.pt) return false;
    if (g.h < 1 || g.w < 1 || g.h + 2 * g.pt < g.kh || g.w + 2 * g.pt < g.kw) return false;
    if (g.oh != (g.h + 2 * g.pt - g.kh) / g.sh + 1 || g.ow != (g.w + 2 * g.pt - g.kw) / g.sw + 1) return false;
    if (g.oh < 1 || g.ow < 1 || g.cip != round_up(g.c_in, 16)) return false;
    const int64_t lim = (int64_t)1 << 31;
    return (int64_t)g.n * g.h * g.w * g.cip < lim && (int64_t)g.n * g.oh * g.ow * g.cip < lim &&
           (int64_t)g.cip * g.kh * g.kw * 4 * DW_MAX_SLABS < lim;
}

hipError_t dwconv_fwd(const ConvGeom& g, const int8_t* x, const int8_t* w, uint32_t* amax, const ActOut& o, int pass,
                      hipStream_t st) {
    return dw_act(g, false, x, w, amax, o, pass, st);
}

hipError_t dwconv_dgrad(const ConvGeom& g, const int8_t* dy, const int8_t* w, uint32_t* amax, const ActOut& o, int pass,
                        hipStream_t st) {
    return dw_act(g, true, dy, w, amax, o, pass, st);
}

int dwconv_wgrad_slabs(const ConvGeom& g) { return dwconv2_ok(g) ? dw_wgrad_plan(g).slabs : 0; }

hipError_t dwconv_wgrad(const ConvGeom& g, const int8_t* x, const int8_t* dy, int32_t* slab, size_t slab_bytes,
                        int* slabs, hipStream_t st, SgdJob* defer) {
    if (!dwconv2_ok(g) || x == nullptr || dy == nullptr || slab == nullptr) return hipErrorInvalidValue;
    const DwWgPlan p = dw_wgrad_plan(g);
    const size_t one = (size_t)g.kh * g.kw * g.cip;  // elements of a slab
    if (p.slabs * one * sizeof(int32_t) > slab_bytes) return hipErrorInvalidValue;
    DwWgArgs a{};
    a.x = x;
    a.dy = dy;
    a.slab = slab;
    a.xbytes = (uint32_t)((int64_t)g.n * g.h * g.w * g.cip);
    a.dbytes = (uint32_t)((int64_t)g.n * g.oh * g.ow * g.cip);
    a.sbytes = (uint32_t)(p.slabs * one * sizeof(int32_t));
    a.h = g.h;
    a.w = g.w;
    a.oh = g.oh;
    a.ow = g.ow;
    a.cp = g.cip;
    a.pad = g.pt;
    a.G = p.G;
    a.GB = p.GB;
    a.R = p.R;
    a.rows = g.n * g.oh;
    a.fgb = make_fastdiv((uint32_t)p.GB);
    a.foh = make_fastdiv((uint32_t)g.oh);
    const dim3 grid((unsigned)p.slabs, (unsigned)p.gy);
    using Kern = void (*)(DwWgArgs);
    const Kern f = g.kh == 3 ? (g.sh == 2 ? dwconv_wgrad_kernel<3, 2> : dwconv_wgrad_kernel<3, 1>)
                             : (g.sh == 2 ? dwconv_wgrad_kernel<5, 2> : dwconv_wgrad_kernel<5, 1>);
    hipLaunchKernelGGL(f, grid, dim3(256), 0, st, a);
    if (slabs != nullptr) *slabs = p.slabs;
    if (defer != nullptr) {  // C-shaped slabs for the update launch's combine
        defer->slab = slab;
        defer->splits = p.slabs;
        defer->slab_stride = (int64_t)one;
        defer->slab_n = (int64_t)one;
        defer->slab_map = 0;
    }
    return hipGetLastError();
}

}  // namespace niti
