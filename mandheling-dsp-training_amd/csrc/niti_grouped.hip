// niti_grouped.hip -- grouped 3x3 conv layers (the kernels and gc_wide(); launched by niti_grouped_host.hip, behind
// gconv_* of niti_kernels.hpp): groups = G >= 2, c_in = c_out =
// G * cg with cg 16, 32 or 64 channels a group, stride 1 or 2 (the stride-2 kernels: below, "stride 2"), one pad
// 0..2 on every side.
//
// The layer is NITI_Conv_Int8 over the block-diagonal dense weight.  A group contracts over 9 cg terms:
// that fits v_mfma_i32_16x16x64_i8, 16 rows x 16 columns over 64 bytes of K, four 16-byte K slots of
// which lane l supplies slot l / 16 of row (A) or column (B) l % 16.  The accumulator, by the ISA's
// table for the 16x16 forms: lane l holds column l % 16, rows 4 (l / 16) + r in register r = 0..3.
//
// Layouts.  Activations NHWC16 [n][h][w][C].  The weight, its int32 gradient and the gradient's slabs
// are [c_out][9][cg]: the OHWI16 form of a dense layer with c_in = cg.  Nothing else exists: no
// transposed weight, no fragment copy.
//
// gconv_act (forward; the input gradient is the same conv on dy with the taps reversed and pad 2 - pad).
// A = the weights (rows: 16 output channels of the group), B = the pixels (columns: 16 consecutive
// output pixels of a row), so a lane's accumulator registers are 4 consecutive channels of one pixel:
// one dword of the int8 output.  Slot map, the same for A and B: slot s = tap * (cg / 16) + c16 is the
// tap's channels 16 c16 .. 16 c16 + 15 (of the input for the forward, of dy for the input gradient);
// MFMA number s / 4 takes it in K slot s % 4, and the slots past 9 cg / 16 are zeros in A.
// A workgroup takes (image, group, 4 output rows, up to 4 strips of 16 columns).  LDS:
//   xs  [c16][6 rows][16 strips + 2 columns][16 bytes]  the input rows with halo, the group's channels;
//       a slot's 16 lanes read 256 contiguous bytes (conflict-free); outside the image: zeros, decided
//       from row and column;
//   wsm [slot][cg rows][16 bytes]                        the group's weights, fragment-major; for the
//       input gradient transposed within the group on the way in (4x4 byte blocks, tr4) and the tap
//       reversed.
// The weight fragments stay in registers at cg 16 (3 MFMAs a tile) and 32 (2 x 5) and are read per
// tile from LDS at cg 64 (4 x 9).  Pass 0 publishes max|acc|, pass 1 reads the range and recomputes,
// requantising by NITI_Conv_Int8.cpp:260-307's rule chosen once per wave: no int32 tensor.
//
// gconv_wgrad.  Per group and tap a cg x cg product over the pixels: A = dy (rows: output channels),
// B = x (columns: input channels), a slot = 16 consecutive pixels of one channel.  A workgroup takes
// one group and a share of the (image, 4 output rows, 4 strips) bands; per band it writes the 4 dy
// rows and 6 x rows into LDS pixel-major (tr4 again: [channel][row][pixel], channel pitches padded so
// that a slot's 16 lanes read conflict-free), zeros outside the image.  K slot q of MFMA k is output
// row q, strip k; the kx shifts of x are v_alignbyte_b32 over an aligned 16-byte read and the dword
// behind it, the ky shifts other rows.  The waves split the 9 (cg / 16)^2 accumulator tiles:
// cg 16: a tap row each (3 tiles, the fourth wave only loads); cg 32: one (o16, i16) pair each, 9 taps;
// cg 64: one o16 each, 4 x 9 = 36 tiles, 144 accumulator registers.  The workgroup writes its group's
// part of one slab; the slab count is a function of the shape alone.
#include <algorithm>

#include "niti_device.hpp"
#include "niti_grouped.hpp"
#include "niti_kernels.hpp"
#include "niti_sgd.hpp"

namespace niti {

namespace {

constexpr int GC_ROWS = 4;    // output rows of a band
constexpr int GC_STRIPS = 4;  // 16-pixel strips of a band, at most
template <int CG, bool DGRAD, int PASS>
__global__ void __launch_bounds__(256) gconv_act_kernel(GcActArgs a) {
    constexpr int NCH = CG / 16;             // 16-channel chunks of a group
    constexpr int NS = 9 * NCH;              // K slots
    constexpr int NK = (NS + 3) / 4;         // MFMAs of a tile
    constexpr int NT = NCH;                  // 16-channel output tiles
    constexpr bool WREG = CG <= 32;          // the weight fragments in registers
    constexpr int TR = GC_ROWS + 2, TWMAX = 16 * GC_STRIPS + 2;
    __shared__ __attribute__((aligned(16))) int8_t xs[NCH * TR * TWMAX * 16];
    __shared__ __attribute__((aligned(16))) int8_t wsm[NS * CG * 16];
    __shared__ uint32_t red[4];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.xbytes), rw = make_rsrc(a.w, a.wbytes);
    uint32_t gm = 0;
    if (PASS == 1) gm = a.amax[lane * MAX_SLOT_STRIDE];

    const int grp = (int)blockIdx.y;
    const int tiles = a.bands * a.segs;
    const int img = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - img * tiles;
    const int band = tile / a.segs, seg = tile - band * a.segs;
    const int oy0 = band * GC_ROWS, s0 = seg * GC_STRIPS;
    const int strips_all = (a.ow + 15) >> 4;
    const int S = min(GC_STRIPS, strips_all - s0);  // this tile's strips
    const int TW = 16 * S + 2;

    // the input tile: rows oy0 - pad .. + 5, columns 16 s0 - pad .. + TW - 1, the group's channels
    for (int e = threadIdx.x; e < TR * TW * NCH; e += 256) {
        const int ch = e % NCH, px = e / NCH;
        const int r = px / TW, c = px - r * TW;
        const int iy = oy0 - a.pad + r, ix = 16 * s0 - a.pad + c;
        const bool ok = iy >= 0 && iy < a.ih && ix >= 0 && ix < a.iw;
        const v4i v = buf_load16(
            rx, ok ? (uint32_t)(((img * a.ih + iy) * a.iw + ix) * a.C + grp * CG + ch * 16) : OOB);
        *(v4i*)(xs + ((ch * TR + r) * TW + c) * 16) = v;
    }
    // the group's weights, fragment-major [slot][row][16]
    if (!DGRAD) {
        // row = output channel o, slot = (tap, 16 input channels): a 16-byte unit of w as it lies
        for (int e = threadIdx.x; e < CG * NS; e += 256) {
            const int o = e / NS, s = e - o * NS;
            const v4i v = buf_load16(rw, (uint32_t)(((grp * CG + o) * NS + s) * 16));
            *(v4i*)(wsm + (s * CG + o) * 16) = v;
        }
    } else {
        // row = input channel i, slot = (reversed tap, 16 output channels): four output channels' 16-byte
        // units of one (tap, i16) transpose into 16 dwords, one per input channel
        for (int e = threadIdx.x; e < 9 * (CG / 4) * NCH; e += 256) {
            const int ic = e % NCH, rest = e / NCH;
            const int oq = rest % (CG / 4), tap = rest / (CG / 4);
            v4i v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                v[r] = buf_load16(rw, (uint32_t)((((grp * CG + 4 * oq + r) * 9 + tap) * NCH + ic) * 16));
            const int s = (8 - tap) * NCH + (oq >> 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int R[4];
                tr4(v[0][j], v[1][j], v[2][j], v[3][j], R);
#pragma unroll
                for (int b = 0; b < 4; ++b) *(int*)(wsm + (s * CG + ic * 16 + 4 * j + b) * 16 + 4 * (oq & 3)) = R[b];
            }
        }
    }
    __syncthreads();

    // this lane's K slots: slot 4 k + q = (tap, c16) reads the tile at (row + ky, column + kx) of plane c16
    int xoff[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int s = 4 * k + q;
        const int tap = s / NCH, ch = s - tap * NCH;
        xoff[k] = s < NS ? ((ch * TR + tap / 3) * TW + tap % 3) * 16 : 0;
    }
    auto wfrag = [&](int t, int k) {
        const int s = 4 * k + q;
        return s < NS ? *(const v4i*)(wsm + (s * CG + 16 * t + col) * 16) : v4i{0, 0, 0, 0};
    };
    v4i wr[WREG ? NT : 1][WREG ? NK : 1];
    if (WREG) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int k = 0; k < NK; ++k) wr[t][k] = wfrag(t, k);
    }

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
    // a wave's units: (row, strip) pairs of the tile
    for (int u = wave; u < GC_ROWS * S; u += 4) {
        const int r = u / S, sx = u - r * S;
        const int oy = oy0 + r, ox = 16 * (s0 + sx) + col;
        if (oy >= a.oh) break;  // (uniform: rows ascend with u)
        const bool valid = ox < a.ow;  // a partial last strip computes masked pixels and stores nothing
        const int8_t* xb = xs + (r * TW + 16 * sx + col) * 16;
        v4i xf[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) xf[k] = *(const v4i*)(xb + xoff[k]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            v4i acc{0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < NK; ++k)
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(WREG ? wr[WREG ? t : 0][WREG ? k : 0] : wfrag(t, k), xf[k],
                                                            acc, 0, 0, 0);
            // acc[e]: pixel `col` of the strip, channel 16 t + 4 q + e of the group
            if (PASS == 0) {
                if (valid)
#pragma unroll
                    for (int e = 0; e < 4; ++e) m = max(m, uabs32(acc[e]));
            } else if (valid) {
                const size_t off = (((size_t)img * a.oh + oy) * a.ow + ox) * a.C + grp * CG + 16 * t + 4 * q;
                uint32_t mk = 0;
                if (a.relu_mask != nullptr) mk = *(const uint32_t*)(a.relu_mask + off);
                uint32_t o = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int32_t v = raw ? (int32_t)(int8_t)acc[e] : psto_fast(acc[e], s);
                    if (a.relu && v < 0) v = 0;
                    if (a.relu_mask != nullptr && (int8_t)(mk >> (8 * e)) <= 0) v = 0;
                    o |= ((uint32_t)v & 0xffu) << (8 * e);
                }
                *(uint32_t*)(a.out + off) = o;
            }
        }
    }

    if (PASS == 0) {
        m = wave_max(m);
        if (lane == 0) red[wave] = m;
        __syncthreads();
        if (threadIdx.x == 0) publish_max(a.amax, max(max(red[0], red[1]), max(red[2], red[3])));
    }
}

template <int CG>
__global__ void __launch_bounds__(256) gconv_wgrad_kernel(GcWgArgs a) {
    constexpr int NCH = CG / 16;
    constexpr int NTI = CG == 64 ? 4 : 1;  // input-channel tiles of a wave
    constexpr int NKY = CG == 16 ? 1 : 3;  // tap rows of a wave
    // pitches in bytes, for 4 strips: a dy row, an x row (16 more: the kx shifts read past the last strip),
    // a channel of each (16 more: a slot's 16 lanes, one channel each, then read conflict-free)
    constexpr int DPMAX = 16 * GC_STRIPS, XPMAX = DPMAX + 16;
    constexpr int XROWS = GC_ROWS + 2;
    __shared__ __attribute__((aligned(16))) int8_t dT[CG * (GC_ROWS * DPMAX + 16)];
    __shared__ __attribute__((aligned(16))) int8_t xT[CG * (XROWS * XPMAX + 16)];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    const int grp = (int)blockIdx.y;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.xbytes), rd = make_rsrc(a.dy, a.dbytes);
    // this wave's tiles: output channels 16 to .., input channels 16 (ti0 + i) .., tap rows ky0 + j
    const int to = CG == 64 ? wave : CG == 32 ? wave >> 1 : 0;
    const int ti0 = CG == 32 ? wave & 1 : 0;
    const int ky0 = CG == 16 ? wave : 0;
    const bool works = CG != 16 || wave < 3;

    v4i acc[NTI][NKY][3];
#pragma unroll
    for (int i = 0; i < NTI; ++i)
#pragma unroll
        for (int j = 0; j < NKY; ++j)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[i][j][kx] = v4i{0, 0, 0, 0};

    const int strips_all = (a.ow + 15) >> 4;
    const int per_img = a.bands * a.segs;
    for (int unit = (int)blockIdx.x; unit < a.units; unit += (int)gridDim.x) {
        const int img = unit / per_img, tile = unit - img * per_img;
        const int band = tile / a.segs, seg = tile - band * a.segs;
        const int oy0 = band * GC_ROWS, s0 = seg * GC_STRIPS;
        const int S = min(GC_STRIPS, strips_all - s0);
        const int DP = 16 * S, XP = DP + 16;
        const int DCH = GC_ROWS * DP + 16, XCH = XROWS * XP + 16;
        __syncthreads();  // (the previous band's reads are over)
        // dy rows oy0 .. + 3, columns 16 s0 .. + DP - 1: four pixels x 16 channels -> 16 dwords of four pixels
        for (int e = threadIdx.x; e < GC_ROWS * (DP / 4) * NCH; e += 256) {
            const int ch = e % NCH, rest = e / NCH;
            const int pq = rest % (DP / 4), r = rest / (DP / 4);
            const int oy = oy0 + r;
            v4i v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int ox = 16 * s0 + 4 * pq + p;
                const bool ok = oy < a.oh && ox < a.ow;
                v[p] = buf_load16(
                    rd, ok ? (uint32_t)(((img * a.oh + oy) * a.ow + ox) * a.C + grp * CG + ch * 16) : OOB);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int R[4];
                tr4(v[0][j], v[1][j], v[2][j], v[3][j], R);
#pragma unroll
                for (int b = 0; b < 4; ++b) *(int*)(dT + (ch * 16 + 4 * j + b) * DCH + r * DP + 4 * pq) = R[b];
            }
        }
        // x rows oy0 - pad .. + 5, columns 16 s0 - pad .. + XP - 1 (position p = column + pad - 16 s0)
        for (int e = threadIdx.x; e < XROWS * (XP / 4) * NCH; e += 256) {
            const int ch = e % NCH, rest = e / NCH;
            const int pq = rest % (XP / 4), r = rest / (XP / 4);
            const int iy = oy0 - a.pad + r;
            v4i v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int ix = 16 * s0 - a.pad + 4 * pq + p;
                const bool ok = iy >= 0 && iy < a.h && ix >= 0 && ix < a.w;
                v[p] = buf_load16(
                    rx, ok ? (uint32_t)(((img * a.h + iy) * a.w + ix) * a.C + grp * CG + ch * 16) : OOB);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int R[4];
                tr4(v[0][j], v[1][j], v[2][j], v[3][j], R);
#pragma unroll
                for (int b = 0; b < 4; ++b) *(int*)(xT + (ch * 16 + 4 * j + b) * XCH + r * XP + 4 * pq) = R[b];
            }
        }
        __syncthreads();
        if (!works) continue;
        // MFMA k: K slot q = output row oy0 + q, strip s0 + k
        for (int k = 0; k < S; ++k) {
            const v4i fa = *(const v4i*)(dT + (16 * to + col) * DCH + q * DP + 16 * k);
#pragma unroll
            for (int i = 0; i < NTI; ++i) {
                const int8_t* xc = xT + (16 * (ti0 + i) + col) * XCH + 16 * k;
#pragma unroll
                for (int j = 0; j < NKY; ++j) {
                    const int8_t* xr = xc + (q + ky0 + j) * XP;
                    const v4i lo = *(const v4i*)xr;
                    const int hi = *(const int*)(xr + 16);
                    const int d[5] = {lo[0], lo[1], lo[2], lo[3], hi};
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        v4i fb = lo;
                        if (kx > 0)
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                fb[e] = (int)__builtin_amdgcn_alignbyte((uint32_t)d[e + 1], (uint32_t)d[e], (uint32_t)kx);
                        acc[i][j][kx] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa, fb, acc[i][j][kx], 0, 0, 0);
                    }
                }
            }
        }
    }

    // acc[i][j][kx][e]: output channel 16 to + 4 q + e, input channel 16 (ti0 + i) + col, tap (ky0 + j, kx)
    if (!works) return;
    int32_t* sl = a.slab + (size_t)blockIdx.x * a.C * 9 * CG;
#pragma unroll
    for (int i = 0; i < NTI; ++i)
#pragma unroll
        for (int j = 0; j < NKY; ++j)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int o = grp * CG + 16 * to + 4 * q + e, tap = 3 * (ky0 + j) + kx;
                    sl[((size_t)o * 9 + tap) * CG + 16 * (ti0 + i) + col] = acc[i][j][kx][e];
                }
}

// ---- stride 2 -------------------------------------------------------------------------------------
// oh = (h + 2 pad - 3) / 2 + 1.  The same MFMA, accumulator layout, slot = (tap, c16) idea, two-pass range
// protocol and slab form; what differs is how the tiles lie in LDS.
//
// gconv2_fwd.  A strip's 16 output pixels read input columns two apart, so the tile (9 rows x 32 S + 1
// columns) is written de-interleaved by the parity of the tile column c = ix + pad - 32 s0:
//   xs [c16][9 rows][2 planes][16 S + 1 columns][16 bytes]
// tap (ky, kx) of output (r, j) is row 2 r + ky, plane kx & 1, column j + (kx >> 1): a slot's 16 lanes read
// 256 contiguous bytes again.  cg 64 takes 2 strips a workgroup (73 KiB of LDS, two workgroups a CU), else 4.
//
// gconv2_dgrad.  With Y = y + pad, X = x + pad, a = Y >> 1, b = X >> 1, the pixel's class (Y & 1, X & 1)
// admits the taps ky = Y & 1 (mod 2), kx = X & 1 (mod 2): dy(a - (ky >> 1), b - (kx >> 1)) for ky, kx even,
// dy(a, b) for 1.  A workgroup takes (image, group, 4 rows of a, up to S strips of 16 b) and all four classes:
//   ds  [c16][5 rows][16 S + 1 columns][16 bytes]   dy rows a0 - 1 .., columns b0 - 1 .., zeros outside dy
//   wsm [tap * cg / 16 + o16][cg rows i][16 bytes]  the group's weights transposed (tr4), taps as they lie
// A class is one instantiation of gc2_dgrad_class: its slots are its own taps x cg / 16, ceil(ntaps cg / 64)
// MFMAs a tile; its 16 pixels sit two columns apart in dx.  A dx row or column no output reads finds only
// zeros in ds.
//
// gconv2_wgrad.  The band is 4 dy rows and the 9 x rows under them, pixel-major through tr4 as at stride 1
// (the transposed LDS read stays the follow-up: the fill is not what bounds this kernel either), x as two
// column-parity planes:
//   xT [channel][9 rows][2 planes][16 S + 16 pixels] (+ 16 bytes a channel: the pitch is an odd count of 16)
// kx = 0 / 1 are aligned 16-byte reads of the even / odd plane, kx = 2 the even plane one pixel on
// (v_alignbyte_b32 by 1), ky row 2 q + ky.  The wave split of the accumulator tiles is the stride-1 one.
constexpr int gc2_strips(int cg) { return cg == 64 ? 2 : 4; }  // strips of a workgroup
constexpr int GC2_XROWS = 2 * GC_ROWS + 1;

// the group's weights into LDS, fragment-major [slot][row][16]: row = output channel, slot = (tap, 16 input
// channels) as w lies, or (TR) row = input channel, slot = (tap, 16 output channels) through tr4
template <int CG, bool TR>
__device__ __forceinline__ void gc2_load_w(const __amdgpu_buffer_rsrc_t rw, int grp, int8_t* wsm) {
    constexpr int NCH = CG / 16, NS = 9 * NCH;
    if (!TR) {
        for (int e = threadIdx.x; e < CG * NS; e += 256) {
            const int o = e / NS, s = e - o * NS;
            *(v4i*)(wsm + (s * CG + o) * 16) = buf_load16(rw, (uint32_t)(((grp * CG + o) * NS + s) * 16));
        }
    } else {
        for (int e = threadIdx.x; e < 9 * (CG / 4) * NCH; e += 256) {
            const int ic = e % NCH, rest = e / NCH;
            const int oq = rest % (CG / 4), tap = rest / (CG / 4);
            v4i v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                v[r] = buf_load16(rw, (uint32_t)((((grp * CG + 4 * oq + r) * 9 + tap) * NCH + ic) * 16));
            const int s = tap * NCH + (oq >> 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int R[4];
                tr4(v[0][j], v[1][j], v[2][j], v[3][j], R);
#pragma unroll
                for (int b = 0; b < 4; ++b) *(int*)(wsm + (s * CG + ic * 16 + 4 * j + b) * 16 + 4 * (oq & 3)) = R[b];
            }
        }
    }
}

template <int CG, int PASS>
__global__ void __launch_bounds__(256) gconv2_fwd_kernel(GcActArgs a) {
    constexpr int NCH = CG / 16, NS = 9 * NCH, NK = (NS + 3) / 4, NT = NCH;
    constexpr bool WREG = CG <= 32;
    constexpr int SMAX = gc2_strips(CG), TR = GC2_XROWS, PWMAX = 16 * SMAX + 1;
    __shared__ __attribute__((aligned(16))) int8_t xs[NCH * TR * 2 * PWMAX * 16];
    __shared__ __attribute__((aligned(16))) int8_t wsm[NS * CG * 16];
    __shared__ uint32_t red[4];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.xbytes), rw = make_rsrc(a.w, a.wbytes);
    uint32_t gm = 0;
    if (PASS == 1) gm = a.amax[lane * MAX_SLOT_STRIDE];

    const int grp = (int)blockIdx.y;
    const int tiles = a.bands * a.segs;
    const int img = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - img * tiles;
    const int band = tile / a.segs, seg = tile - band * a.segs;
    const int oy0 = band * GC_ROWS, s0 = seg * SMAX;
    const int S = min(SMAX, ((a.ow + 15) >> 4) - s0);
    const int PW = 16 * S + 1;

    // the input tile: rows 2 oy0 - pad .. + 8, tile columns c = 0 .. 32 S at 32 s0 - pad + c, plane c & 1
    // (column 32 S + 1, the odd plane's last, is read by no tap: zeros)
    for (int e = threadIdx.x; e < TR * 2 * PW * NCH; e += 256) {
        const int ch = e % NCH, px = e / NCH;
        const int r = px / (2 * PW), c = px - r * 2 * PW;
        const int iy = 2 * oy0 - a.pad + r, ix = 32 * s0 - a.pad + c;
        const bool ok = c <= 32 * S && iy >= 0 && iy < a.ih && ix >= 0 && ix < a.iw;
        const v4i v = buf_load16(
            rx, ok ? (uint32_t)(((img * a.ih + iy) * a.iw + ix) * a.C + grp * CG + ch * 16) : OOB);
        *(v4i*)(xs + (((ch * TR + r) * 2 + (c & 1)) * PW + (c >> 1)) * 16) = v;
    }
    gc2_load_w<CG, false>(rw, grp, wsm);
    __syncthreads();

    // slot 4 k + q = (tap, c16): row ky, plane kx & 1, column kx >> 1 of plane c16, from the unit's corner
    int xoff[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int s = 4 * k + q;
        const int tap = s / NCH, ch = s - tap * NCH;
        const int ky = tap / 3, kx = tap - 3 * ky;
        xoff[k] = s < NS ? (((ch * TR + ky) * 2 + (kx & 1)) * PW + (kx >> 1)) * 16 : 0;
    }
    auto wfrag = [&](int t, int k) {
        const int s = 4 * k + q;
        return s < NS ? *(const v4i*)(wsm + (s * CG + 16 * t + col) * 16) : v4i{0, 0, 0, 0};
    };
    v4i wr[WREG ? NT : 1][WREG ? NK : 1];
    if (WREG) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int k = 0; k < NK; ++k) wr[t][k] = wfrag(t, k);
    }
    const Gc2Quant z = gc2_quant<PASS>(a, gm);

    uint32_t m = 0;
    for (int u = wave; u < GC_ROWS * S; u += 4) {
        const int r = u / S, sx = u - r * S;
        const int oy = oy0 + r, ox = 16 * (s0 + sx) + col;
        if (oy >= a.oh) break;  // (uniform: rows ascend with u)
        const int8_t* xb = xs + (2 * r * 2 * PW + 16 * sx + col) * 16;
        v4i xf[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) xf[k] = *(const v4i*)(xb + xoff[k]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            v4i acc{0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < NK; ++k)
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(WREG ? wr[WREG ? t : 0][WREG ? k : 0] : wfrag(t, k), xf[k],
                                                            acc, 0, 0, 0);
            // a partial last strip computes masked pixels and stores nothing
            if (ox < a.ow)
                gc2_emit<PASS>(a, acc, (((size_t)img * a.oh + oy) * a.ow + ox) * a.C + grp * CG + 16 * t + 4 * q, z, m);
        }
    }
    gc2_publish<PASS>(a, m, red);
}

// One parity class (PY, PX) of the input gradient over the wave's units of the tile: dx pixels (2 A + PY - pad,
// 2 B + PX - pad) for A = a0 + r, B = b0 + 16 sx + col
template <int CG, int PASS, int PY, int PX>
__device__ __forceinline__ void gc2_dgrad_class(const GcActArgs& a, const int8_t* ds, const int8_t* wsm, int S, int img,
                                                int grp, int a0, int b0, int na, Gc2Quant z, uint32_t& m) {
    constexpr int NCH = CG / 16, NTX = PX ? 1 : 2, NTAP = (PY ? 1 : 2) * NTX;
    constexpr int NS = NTAP * NCH, NK = (NS + 3) / 4, NT = NCH;
    constexpr bool WREG = CG <= 32;
    constexpr int TR = GC_ROWS + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    const int TW = 16 * S + 1;
    // slot 4 k + q = (the class's tap (jy, jx), c16): ky = 2 jy or 1, kx = 2 jx or 1; dy at (A - jy, B - jx) is
    // tile (r + 1 - jy, 16 sx + col + 1 - jx)
    int xoff[NK], wslot[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int s = 4 * k + q;
        const int t = s / NCH, ch = s - t * NCH;
        const int jy = t / NTX, jx = t - jy * NTX;
        const int ky = PY ? 1 : 2 * jy, kx = PX ? 1 : 2 * jx;
        xoff[k] = s < NS ? ((ch * TR + 1 - jy) * TW + 1 - jx) * 16 : 0;
        wslot[k] = s < NS ? (3 * ky + kx) * NCH + ch : -1;
    }
    auto wfrag = [&](int t, int k) {
        return wslot[k] >= 0 ? *(const v4i*)(wsm + (wslot[k] * CG + 16 * t + col) * 16) : v4i{0, 0, 0, 0};
    };
    v4i wr[WREG ? NT : 1][WREG ? NK : 1];
    if (WREG) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int k = 0; k < NK; ++k) wr[t][k] = wfrag(t, k);
    }
    for (int u = wave; u < GC_ROWS * S; u += 4) {
        const int r = u / S, sx = u - r * S;
        if (a0 + r >= na) break;  // (uniform: rows ascend with u)
        const int y = 2 * (a0 + r) + PY - a.pad, x = 2 * (b0 + 16 * sx + col) + PX - a.pad;
        if (y < 0 || y >= a.oh) continue;  // (uniform)
        const int8_t* xb = ds + (r * TW + 16 * sx + col) * 16;
        v4i xf[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) xf[k] = *(const v4i*)(xb + xoff[k]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            v4i acc{0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < NK; ++k)
                acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(WREG ? wr[WREG ? t : 0][WREG ? k : 0] : wfrag(t, k), xf[k],
                                                            acc, 0, 0, 0);
            // acc[e]: the pixel of lane `col`, input channel 16 t + 4 q + e of the group
            if (x >= 0 && x < a.ow)
                gc2_emit<PASS>(a, acc, (((size_t)img * a.oh + y) * a.ow + x) * a.C + grp * CG + 16 * t + 4 * q, z, m);
        }
    }
}

// a: x = dy [n][ih][iw][C], out = dx [n][oh][ow][C], pad = the layer's; bands / segs over a and b
template <int CG, int PASS>
__global__ void __launch_bounds__(256) gconv2_dgrad_kernel(GcActArgs a) {
    constexpr int NCH = CG / 16, NS = 9 * NCH;
    constexpr int SMAX = gc2_strips(CG), TR = GC_ROWS + 1, TWMAX = 16 * SMAX + 1;
    __shared__ __attribute__((aligned(16))) int8_t ds[NCH * TR * TWMAX * 16];
    __shared__ __attribute__((aligned(16))) int8_t wsm[NS * CG * 16];
    __shared__ uint32_t red[4];

    const int lane = threadIdx.x & 63;
    const __amdgpu_buffer_rsrc_t rd = make_rsrc(a.x, a.xbytes), rw = make_rsrc(a.w, a.wbytes);
    uint32_t gm = 0;
    if (PASS == 1) gm = a.amax[lane * MAX_SLOT_STRIDE];

    const int grp = (int)blockIdx.y;
    const int tiles = a.bands * a.segs;
    const int img = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - img * tiles;
    const int band = tile / a.segs, seg = tile - band * a.segs;
    const int na = ((a.oh - 1 + a.pad) >> 1) + 1, nb = ((a.ow - 1 + a.pad) >> 1) + 1;
    const int a0 = band * GC_ROWS, s0 = seg * SMAX, b0 = 16 * s0;
    const int S = min(SMAX, ((nb + 15) >> 4) - s0);
    const int TW = 16 * S + 1;

    for (int e = threadIdx.x; e < TR * TW * NCH; e += 256) {
        const int ch = e % NCH, px = e / NCH;
        const int r = px / TW, c = px - r * TW;
        const int oy = a0 - 1 + r, ox = b0 - 1 + c;
        const bool ok = oy >= 0 && oy < a.ih && ox >= 0 && ox < a.iw;
        const v4i v = buf_load16(
            rd, ok ? (uint32_t)(((img * a.ih + oy) * a.iw + ox) * a.C + grp * CG + ch * 16) : OOB);
        *(v4i*)(ds + ((ch * TR + r) * TW + c) * 16) = v;
    }
    gc2_load_w<CG, true>(rw, grp, wsm);
    __syncthreads();

    const Gc2Quant z = gc2_quant<PASS>(a, gm);
    uint32_t m = 0;
    gc2_dgrad_class<CG, PASS, 0, 0>(a, ds, wsm, S, img, grp, a0, b0, na, z, m);
    gc2_dgrad_class<CG, PASS, 0, 1>(a, ds, wsm, S, img, grp, a0, b0, na, z, m);
    gc2_dgrad_class<CG, PASS, 1, 0>(a, ds, wsm, S, img, grp, a0, b0, na, z, m);
    gc2_dgrad_class<CG, PASS, 1, 1>(a, ds, wsm, S, img, grp, a0, b0, na, z, m);
    gc2_publish<PASS>(a, m, red);
}

template <int CG>
__global__ void __launch_bounds__(256) gconv2_wgrad_kernel(GcWgArgs a) {
    constexpr int NCH = CG / 16;
    constexpr int NTI = CG == 64 ? 4 : 1;  // input-channel tiles of a wave
    constexpr int NKY = CG == 16 ? 1 : 3;  // tap rows of a wave
    constexpr int SMAX = gc2_strips(CG);
    constexpr int DPMAX = 16 * SMAX, XPMAX = DPMAX + 16;  // a dy row; a plane's row (the kx = 2 shift reads on)
    __shared__ __attribute__((aligned(16))) int8_t dT[CG * (GC_ROWS * DPMAX + 16)];
    __shared__ __attribute__((aligned(16))) int8_t xT[CG * (GC2_XROWS * 2 * XPMAX + 16)];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    const int grp = (int)blockIdx.y;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.xbytes), rd = make_rsrc(a.dy, a.dbytes);
    const int to = CG == 64 ? wave : CG == 32 ? wave >> 1 : 0;
    const int ti0 = CG == 32 ? wave & 1 : 0;
    const int ky0 = CG == 16 ? wave : 0;
    const bool works = CG != 16 || wave < 3;

    v4i acc[NTI][NKY][3];
#pragma unroll
    for (int i = 0; i < NTI; ++i)
#pragma unroll
        for (int j = 0; j < NKY; ++j)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[i][j][kx] = v4i{0, 0, 0, 0};

    const int strips_all = (a.ow + 15) >> 4;
    const int per_img = a.bands * a.segs;
    for (int unit = (int)blockIdx.x; unit < a.units; unit += (int)gridDim.x) {
        const int img = unit / per_img, tile = unit - img * per_img;
        const int band = tile / a.segs, seg = tile - band * a.segs;
        const int oy0 = band * GC_ROWS, s0 = seg * SMAX;
        const int S = min(SMAX, strips_all - s0);
        const int DP = 16 * S, XP = DP + 16;
        const int DCH = GC_ROWS * DP + 16, XCH = GC2_XROWS * 2 * XP + 16;
        __syncthreads();  // (the previous band's reads are over)
        for (int e = threadIdx.x; e < GC_ROWS * (DP / 4) * NCH; e += 256) {
            const int ch = e % NCH, rest = e / NCH;
            const int pq = rest % (DP / 4), r = rest / (DP / 4);
            const int oy = oy0 + r;
            v4i v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int ox = 16 * s0 + 4 * pq + p;
                const bool ok = oy < a.oh && ox < a.ow;
                v[p] = buf_load16(
                    rd, ok ? (uint32_t)(((img * a.oh + oy) * a.ow + ox) * a.C + grp * CG + ch * 16) : OOB);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int R[4];
                tr4(v[0][j], v[1][j], v[2][j], v[3][j], R);
#pragma unroll
                for (int b = 0; b < 4; ++b) *(int*)(dT + (ch * 16 + 4 * j + b) * DCH + r * DP + 4 * pq) = R[b];
            }
        }
        // x rows 2 oy0 - pad .. + 8; plane `par`, pixel i is tile column 2 i + par at 32 s0 - pad; four pixels of
        // a plane x 16 channels -> 16 dwords; past pixel 16 S nothing is read for a product: zeros
        for (int e = threadIdx.x; e < GC2_XROWS * 2 * (XP / 4) * NCH; e += 256) {
            const int ch = e % NCH, rest = e / NCH;
            const int pq = rest % (XP / 4), rp = rest / (XP / 4);
            const int r = rp >> 1, par = rp & 1;
            const int iy = 2 * oy0 - a.pad + r;
            v4i v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int i = 4 * pq + p;
                const int ix = 32 * s0 - a.pad + 2 * i + par;
                const bool ok = i <= 16 * S && iy >= 0 && iy < a.h && ix >= 0 && ix < a.w;
                v[p] = buf_load16(
                    rx, ok ? (uint32_t)(((img * a.h + iy) * a.w + ix) * a.C + grp * CG + ch * 16) : OOB);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int R[4];
                tr4(v[0][j], v[1][j], v[2][j], v[3][j], R);
#pragma unroll
                for (int b = 0; b < 4; ++b) *(int*)(xT + (ch * 16 + 4 * j + b) * XCH + rp * XP + 4 * pq) = R[b];
            }
        }
        __syncthreads();
        if (!works) continue;
        // MFMA k: K slot q = output row oy0 + q, strip s0 + k
        for (int k = 0; k < S; ++k) {
            const v4i fa = *(const v4i*)(dT + (16 * to + col) * DCH + q * DP + 16 * k);
#pragma unroll
            for (int i = 0; i < NTI; ++i) {
                const int8_t* xc = xT + (16 * (ti0 + i) + col) * XCH + 16 * k;
#pragma unroll
                for (int j = 0; j < NKY; ++j) {
                    const int8_t* xr = xc + (2 * q + ky0 + j) * 2 * XP;  // the even plane; the odd one XP on
                    const v4i ev = *(const v4i*)xr;
                    const int hi = *(const int*)(xr + 16);
                    const v4i od = *(const v4i*)(xr + XP);
                    const int d[5] = {ev[0], ev[1], ev[2], ev[3], hi};
                    v4i e2;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        e2[e] = (int)__builtin_amdgcn_alignbyte((uint32_t)d[e + 1], (uint32_t)d[e], 1u);
                    acc[i][j][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa, ev, acc[i][j][0], 0, 0, 0);
                    acc[i][j][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa, od, acc[i][j][1], 0, 0, 0);
                    acc[i][j][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa, e2, acc[i][j][2], 0, 0, 0);
                }
            }
        }
    }

    // acc[i][j][kx][e]: output channel 16 to + 4 q + e, input channel 16 (ti0 + i) + col, tap (ky0 + j, kx)
    if (!works) return;
    int32_t* sl = a.slab + (size_t)blockIdx.x * a.C * 9 * CG;
#pragma unroll
    for (int i = 0; i < NTI; ++i)
#pragma unroll
        for (int j = 0; j < NKY; ++j)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int o = grp * CG + 16 * to + 4 * q + e, tap = 3 * (ky0 + j) + kx;
                    sl[((size_t)o * 9 + tap) * CG + 16 * (ti0 + i) + col] = acc[i][j][kx][e];
                }
}

// the column segments of `cols` unit pixels: 4 strips a workgroup at stride 1, gc2_strips(cg) at stride 2
int gc_segs(int cols, int cg, int stride) {
    const int s = stride == 2 ? gc2_strips(cg) : GC_STRIPS;
    return ((cols + 15) / 16 + s - 1) / s;
}

GcActKern gc_act_kernel(int cg, int stride, bool dgrad, int pass) {
    if (stride == 2) {
        static const GcActKern tab2[3][2][2] = {
            {{gconv2_fwd_kernel<16, 0>, gconv2_fwd_kernel<16, 1>}, {gconv2_dgrad_kernel<16, 0>, gconv2_dgrad_kernel<16, 1>}},
            {{gconv2_fwd_kernel<32, 0>, gconv2_fwd_kernel<32, 1>}, {gconv2_dgrad_kernel<32, 0>, gconv2_dgrad_kernel<32, 1>}},
            {{gconv2_fwd_kernel<64, 0>, gconv2_fwd_kernel<64, 1>}, {gconv2_dgrad_kernel<64, 0>, gconv2_dgrad_kernel<64, 1>}}};
        return tab2[cg == 16 ? 0 : cg == 32 ? 1 : 2][dgrad ? 1 : 0][pass];
    }
    static const GcActKern tab[3][2][2] = {
        {{gconv_act_kernel<16, false, 0>, gconv_act_kernel<16, false, 1>},
         {gconv_act_kernel<16, true, 0>, gconv_act_kernel<16, true, 1>}},
        {{gconv_act_kernel<32, false, 0>, gconv_act_kernel<32, false, 1>},
         {gconv_act_kernel<32, true, 0>, gconv_act_kernel<32, true, 1>}},
        {{gconv_act_kernel<64, false, 0>, gconv_act_kernel<64, false, 1>},
         {gconv_act_kernel<64, true, 0>, gconv_act_kernel<64, true, 1>}}};
    return tab[cg == 16 ? 0 : cg == 32 ? 1 : 2][dgrad ? 1 : 0][pass];
}

GcWgKern gc_wgrad_kernel(int cg, int stride) {
    return stride == 2 ? (cg == 16 ? gconv2_wgrad_kernel<16> : cg == 32 ? gconv2_wgrad_kernel<32> : gconv2_wgrad_kernel<64>)
           : cg == 16  ? gconv_wgrad_kernel<16>
           : cg == 32  ? gconv_wgrad_kernel<32>
                       : gconv_wgrad_kernel<64>;
}

}  // namespace

// a workgroup a group; the weight gradient one slab a workgroup
const GcKernels& gc_wide() {
    static const GcKernels k = {gc_segs, [](int, int groups) { return (unsigned)groups; }, [](int) { return 1u; },
                                0,       gc_act_kernel,                                    gc_wgrad_kernel};
    return k;
}

}  // namespace niti
