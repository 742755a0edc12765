// niti_grouped_packed.hip -- grouped 3x3 conv layers at the group widths the other two families leave out
// (the kernels and gc_packed(); launched by niti_grouped_host.hip): cg a multiple of 8 from 24 to 128 but 32 and 64, groups = G >= 2, c_in =
// c_out = C = G * cg, stride 1 or 2, one pad 0..2 on every side.  What most of the RegNets run (cg 24, 40, 48, 56,
// 112, 120, 128).  Semantics, the two-pass range protocol, the ActOut fields and the slab protocol are
// niti_grouped.hip's; the kernels are their own.
//
// Layouts.  Activations NHWC16 [n][h][w][cp], cp = C rounded up to 16 (C = 72: cp = 80): the padding channels are
// never read and pass 1 writes them as zeros.  The weight, its int32 gradient and the gradient's slabs are
// [c_out][9][cg], unpadded: a weight row is 9 cg bytes, 8-byte aligned.
//
// K packed across taps.  For one output channel the contraction is the row's 9 cg contiguous bytes [tap][c].  The
// row is cut into 64-byte v_mfma_i32_16x16x64_i8 chunks and 16-byte lane slots with no regard to tap boundaries:
// NK = ceil(9 cg / 64) issues per 16x16 tile (cg 24: 4, where padding the width to 32 takes 5); only the last chunk
// carries zeros, and only in A.  Because cg % 8 == 0 every slot is two 8-byte halves, each inside one (tap,
// 8-channel chunk): a lane's B operand is two 8-byte LDS reads at offsets from a per-lane table xoff[k][half],
// computed once before the tile loop from (tap, c8) -> (row + ky, column + kx, plane c8).  At stride 2 the table is
// the same with the columns split by parity (below).
//
// gcp_act (forward; input gradient at stride 1: the same conv on dy, taps reversed, pad 2 - pad).  A = weights (16
// output channels of one group; ceil(cg / 16) tiles a group, the last one's rows past cg zeros in A and never
// stored, so no tile straddles two groups), B = 16 consecutive output pixels of a row.  A workgroup takes (image,
// group, 4 output rows, S strips of 16 columns), keeps the input tile resident and loops stages of 32 output
// channels (two tiles) over it.  LDS:
//   xs  [c8][rows][columns][8 bytes]             stride 1: 6 rows x 16 S + 2 columns
//   xs  [c8][rows][parity][column / 2][8 bytes]  stride 2: 9 rows x 2 planes x 16 S + 1 columns; tap kx of pixel j is
//                                                plane kx & 1, column j + (kx >> 1)
//   wsm [16-byte slot of the row][32 rows][16]   one stage: the rows' bytes as they lie (8-byte loads; the global
//                                                row is only 8-byte aligned, the LDS slot is 16), zeros past 9 cg
//                                                and past row cg; A is one aligned 16-byte read.  Input gradient:
//                                                transposed within the group on the way in (tr4 on 4x4 bytes).
// Bank conflicts: the 16 lanes of a half-slot share (tap, c8) and take consecutive pixels, so with either layout
// they read 128 contiguous bytes, 8-byte aligned: each of 32 dword banks once.  Checked by enumerating, on the host,
// (address / 4) % 32 of the 16 lanes for every width, stride, chunk, quarter and half of the table: all 32 banks
// distinct in every case.  A's 16 lanes of a slot read 256 contiguous bytes, as in niti_grouped.hip.
// S = 4 / stride (cg <= 56), 2 / stride (cg >= 72).  LDS, xs + wsm in KiB (stride 1 / stride 2), by cg:
//   24: 9.3 + 8 / 14 + 8;  40: 15.5 + 12 / 23 + 12;  48: 18.6 + 14 / 28 + 14;  56: 21.7 + 16 / 32 + 16;
//   72: 14.3 + 22 / 21 + 22;  80: 16 + 24 / 24 + 24;  88: 17.5 + 26 / 26 + 26;  96: 19 + 28 / 29 + 28;
//   104: 21 + 30 / 31 + 30;  112: 22 + 32 / 33 + 32;  120: 24 + 34 / 36 + 34;  128: 25.5 + 36 / 38 + 36.
//
// gcp_dgrad2 (input gradient at stride 2).  niti_grouped.hip's parity classes: Y = y + pad, X = x + pad, class
// (Y & 1, X & 1) admits the taps of that parity, dy((Y >> 1) - (ky >> 1), (X >> 1) - (kx >> 1)).  The dy tile is
// [c8][5 rows][16 S + 1 columns][8]; the weights lie transposed, all 9 taps, as above.  A class packs K across its own
// taps (4, 2, 2 or 1 of them: ceil(ntaps cg / 64) issues), so both operands are half-slot reads from per-lane
// tables; a half past the class's bytes reads A in the zero tail of the row.  A dx row or column no output reads
// finds only zeros in the tile and is written as zeros.
//
// gcp_wgrad.  Per group and tap a cg x cg product over the pixels, as gconv_wgrad: dy and x pixel-major in LDS
// through tr4, [channel][row][pixel], K slot = 16 pixels of a row, the kx shifts by v_alignbyte_b32 (stride 2: two
// column-parity planes).  Channels are padded to 16 ceil(cg / 16) with zero rows in LDS: M / N waste only, K is
// pixels.  The ceil(cg / 16)^2 x 9 tiles split into items (o16, block of up to NTI i16 tiles, all 9 taps): NTI = 1
// (cg 24), cg / 16 rounded up (cg 40..56), 4 above, so an item is at most 144 accumulator registers.  A wave takes
// one item; four items a workgroup, the workgroups of one (slab, group) along gridDim.z (1 up to cg 56, 3 at cg
// 72..96, 4 above), each staging the band itself.  Slabs [slabs][c_out][9][cg]; the count is a function of the
// shape alone.
#include <algorithm>

#include "niti_device.hpp"
#include "niti_grouped.hpp"
#include "niti_kernels.hpp"
#include "niti_sgd.hpp"

namespace niti {

namespace {

constexpr int GP_ROWS = 4;  // output rows of a band
constexpr int gp_strips(int cg, int stride) { return (cg <= 64 ? 4 : 2) / stride; }  // 16-pixel strips of a band
constexpr int gp_wg_nti(int mt) { return mt <= 2 ? 1 : mt <= 4 ? mt : 4; }           // i16 tiles of a wgrad item

__device__ __forceinline__ v2i buf_load8(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_bit_cast(v2i, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0));
}
__device__ __forceinline__ v4i mfma64(v4i a, v4i b, v4i c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }
__device__ __forceinline__ v4i lds2x8(const int8_t* lo, const int8_t* hi) {
    const v2i l = *(const v2i*)lo, h = *(const v2i*)hi;
    return v4i{l[0], l[1], h[0], h[1]};
}

// Stage `st` (A rows 32 st .. 32 st + 31 of the group) into wsm [slot][32 rows][16].  !TR: row = output channel,
// its 9 cg bytes as they lie.  TR: row = input channel i, byte (tap' cg + o) = w[o][tap][i] with tap' = 8 - tap
// (REV) or tap; 4 output channels x 8 input channels go through tr4 into 8 dwords.  Zeros past 9 cg and past row cg.
template <int CG, bool TR, bool REV>
__device__ __forceinline__ void gp_load_w(const __amdgpu_buffer_rsrc_t rw, int grp, int st, int8_t* wsm) {
    constexpr int KB = 9 * CG, NH = 8 * ((KB + 63) / 64);  // bytes of a row, 8-byte halves of its padded string
    if (!TR) {
        for (int e = threadIdx.x; e < 32 * NH; e += 256) {
            const int rr = e / NH, H = e - rr * NH;
            const bool ok = 32 * st + rr < CG && 8 * H < KB;
            const v2i v = buf_load8(rw, ok ? (uint32_t)((grp * CG + 32 * st + rr) * KB + 8 * H) : OOB);
            *(v2i*)(wsm + ((H >> 1) * 32 + rr) * 16 + 8 * (H & 1)) = v;
        }
    } else {
        for (int e = threadIdx.x; e < 32 * (NH - KB / 8); e += 256) {
            const int rr = e & 31, H = KB / 8 + (e >> 5);
            *(v2i*)(wsm + ((H >> 1) * 32 + rr) * 16 + 8 * (H & 1)) = v2i{0, 0};
        }
        for (int e = threadIdx.x; e < 9 * (CG / 4) * 4; e += 256) {
            const int i8 = e & 3, rest = e >> 2;
            const int oq = rest % (CG / 4), tap = rest / (CG / 4);
            const int i0 = 32 * st + 8 * i8;
            v2i v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                v[k] = buf_load8(rw, i0 < CG ? (uint32_t)(((grp * CG + 4 * oq + k) * 9 + tap) * CG + i0) : OOB);
            const int p = (REV ? 8 - tap : tap) * CG + 4 * oq;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                int R[4];
                tr4(v[0][j], v[1][j], v[2][j], v[3][j], R);
#pragma unroll
                for (int b = 0; b < 4; ++b) *(int*)(wsm + ((p >> 4) * 32 + 8 * i8 + 4 * j + b) * 16 + (p & 15)) = R[b];
            }
        }
    }
}

// pass 1: the padding channels C .. cp - 1 (8 bytes, where C is no multiple of 16) of the workgroup's output pixels,
// by the last group's workgroups
__device__ __forceinline__ void gp_zero_pad(const GcActArgs& a, int img, int y0, int ny, int x0, int nx) {
    if (a.cp == a.C || blockIdx.y != gridDim.y - 1) return;
    for (int e = threadIdx.x; e < ny * nx; e += 256) {
        const int y = y0 + e / nx, x = x0 + e % nx;
        if (y >= 0 && y < a.oh && x >= 0 && x < a.ow)
            *(v2i*)(a.out + (((size_t)img * a.oh + y) * a.ow + x) * a.cp + a.C) = v2i{0, 0};
    }
}

template <int CG, int STRIDE, bool DGRAD, int PASS>
__global__ void __launch_bounds__(256) gcp_act_kernel(GcActArgs a) {
    static_assert(!(STRIDE == 2 && DGRAD), "gcp_dgrad2_kernel");
    constexpr int C8 = CG / 8, KB = 9 * CG, NK = (KB + 63) / 64, MT = (CG + 15) / 16, NST = (MT + 1) / 2;
    constexpr int SMAX = gp_strips(CG, STRIDE), TR = STRIDE * (GP_ROWS - 1) + 3;
    constexpr int PWMAX = STRIDE == 1 ? 16 * SMAX + 2 : 16 * SMAX + 1;  // columns of a plane
    __shared__ __attribute__((aligned(16))) int8_t xs[C8 * TR * STRIDE * PWMAX * 8];
    __shared__ __attribute__((aligned(16))) int8_t wsm[4 * NK * 32 * 16];
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
    const int oy0 = band * GP_ROWS, s0 = seg * SMAX;
    const int S = min(SMAX, ((a.ow + 15) >> 4) - s0);  // this tile's strips
    const int PW = STRIDE == 1 ? 16 * S + 2 : 16 * S + 1;
    const int tc = STRIDE == 1 ? PW : 32 * S + 1;  // tile columns (stride 2: the odd plane's last is read by no tap)

    // the input tile: rows STRIDE oy0 - pad .., columns STRIDE 16 s0 - pad .., the group's channels in 8-byte parts
    for (int e = threadIdx.x; e < TR * tc * C8; e += 256) {
        const int c8 = e % C8, px = e / C8;
        const int r = px / tc, c = px - r * tc;
        const int iy = STRIDE * oy0 - a.pad + r, ix = STRIDE * 16 * s0 - a.pad + c;
        const bool ok = iy >= 0 && iy < a.ih && ix >= 0 && ix < a.iw;
        const v2i v = buf_load8(rx, ok ? (uint32_t)(((img * a.ih + iy) * a.iw + ix) * a.cp + grp * CG + 8 * c8) : OOB);
        const int cell = STRIDE == 1 ? (c8 * TR + r) * PW + c : ((c8 * TR + r) * 2 + (c & 1)) * PW + (c >> 1);
        *(v2i*)(xs + cell * 8) = v;
    }

    // this lane's half-slots: half h of slot 4 k + q is bytes 8 H .. 8 H + 7 of the row, H = 2 (4 k + q) + h, inside
    // (tap, c8): the tile at (row + ky, column + kx) of plane c8, from the unit's corner.  Past 9 cg: A is zeros.
    int xoff[NK][2];
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = 8 * (2 * (4 * k + q) + h);
            const int tap = p / CG, c8 = (p - tap * CG) >> 3;
            const int ky = tap / 3, kx = tap - 3 * ky;
            const int cell = STRIDE == 1 ? (c8 * TR + ky) * PW + kx : ((c8 * TR + ky) * 2 + (kx & 1)) * PW + (kx >> 1);
            xoff[k][h] = p < KB ? cell * 8 : 0;
        }
    const Gc2Quant z = gc2_quant<PASS>(a, gm);

    uint32_t m = 0;
    for (int st = 0; st < NST; ++st) {
        __syncthreads();  // (the tile is written; the previous stage's reads are over)
        gp_load_w<CG, DGRAD, true>(rw, grp, st, wsm);
        __syncthreads();
        // a wave's units: (row, strip) pairs of the tile
        for (int u = wave; u < GP_ROWS * S; u += 4) {
            const int r = u / S, sx = u - r * S;
            const int oy = oy0 + r, ox = 16 * (s0 + sx) + col;
            if (oy >= a.oh) break;  // (uniform: rows ascend with u)
            const int8_t* xb = xs + (STRIDE * r * STRIDE * PW + 16 * sx + col) * 8;
            v4i acc[2] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}};
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const v4i fb = lds2x8(xb + xoff[k][0], xb + xoff[k][1]);
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    if (2 * st + t < MT) acc[t] = mfma64(*(const v4i*)(wsm + ((4 * k + q) * 32 + 16 * t + col) * 16), fb, acc[t]);
            }
            // acc[t][e]: pixel `col` of the strip, channel 32 st + 16 t + 4 q + e of the group; a partial last strip
            // computes masked pixels and stores nothing
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int c = 32 * st + 16 * t + 4 * q;
                if (c < CG && ox < a.ow)
                    gc2_emit<PASS>(a, acc[t], (((size_t)img * a.oh + oy) * a.ow + ox) * a.cp + grp * CG + c, z, m);
            }
        }
    }
    if (PASS == 1) gp_zero_pad(a, img, oy0, GP_ROWS, 16 * s0, 16 * S);
    gc2_publish<PASS>(a, m, red);
}

// One parity class (PY, PX) of the stride-2 input gradient over the wave's units: dx pixels (2 Ay + PY - pad,
// 2 Bx + PX - pad) for Ay = a0 + r, Bx = b0 + 16 sx + col, input channels 32 st + 16 t + 4 q .. of the group.  The
// class's K string is its taps (jy, jx) -> ky = 2 jy or 1, kx = 2 jx or 1, cg bytes each: dy(Ay - jy, Bx - jx) =
// tile (r + 1 - jy, 16 sx + col + 1 - jx).
template <int CG, int PASS, int PY, int PX>
__device__ __forceinline__ void gcp_dgrad2_class(const GcActArgs& a, const int8_t* ds, const int8_t* wsm, int S, int img,
                                                 int grp, int st, int a0, int b0, int na, Gc2Quant z, uint32_t& m) {
    constexpr int KB = 9 * CG, MT = (CG + 15) / 16;
    constexpr int NTX = PX ? 1 : 2, NTAP = (PY ? 1 : 2) * NTX, KC = NTAP * CG, NK = (KC + 63) / 64;
    constexpr int TR = GP_ROWS + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    const int TW = 16 * S + 1;
    int xoff[NK][2], woff[NK][2];
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = 8 * (2 * (4 * k + q) + h);
            const int t = p / CG, o = p - t * CG;
            const int jy = t / NTX, jx = t - jy * NTX;
            const int ky = PY ? 1 : 2 * jy, kx = PX ? 1 : 2 * jx;
            const int pa = p < KC ? (3 * ky + kx) * CG + o : KB;  // in the row of all 9 taps; KB: its zero tail
            xoff[k][h] = p < KC ? (((o >> 3) * TR + 1 - jy) * TW + 1 - jx) * 8 : 0;
            woff[k][h] = ((pa >> 4) * 32 + col) * 16 + (pa & 8);
        }
    for (int u = wave; u < GP_ROWS * S; u += 4) {
        const int r = u / S, sx = u - r * S;
        if (a0 + r >= na) break;  // (uniform: rows ascend with u)
        const int y = 2 * (a0 + r) + PY - a.pad, x = 2 * (b0 + 16 * sx + col) + PX - a.pad;
        if (y < 0 || y >= a.oh) continue;  // (uniform)
        const int8_t* xb = ds + (r * TW + 16 * sx + col) * 8;
        v4i acc[2] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}};
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const v4i fb = lds2x8(xb + xoff[k][0], xb + xoff[k][1]);
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (2 * st + t < MT)
                    acc[t] = mfma64(lds2x8(wsm + woff[k][0] + 256 * t, wsm + woff[k][1] + 256 * t), fb, acc[t]);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int c = 32 * st + 16 * t + 4 * q;
            if (c < CG && x >= 0 && x < a.ow)
                gc2_emit<PASS>(a, acc[t], (((size_t)img * a.oh + y) * a.ow + x) * a.cp + grp * CG + c, z, m);
        }
    }
}

// a: x = dy [n][ih][iw][cp], out = dx [n][oh][ow][cp], pad = the layer's; bands / segs over (Y >> 1, X >> 1)
template <int CG, int PASS>
__global__ void __launch_bounds__(256) gcp_dgrad2_kernel(GcActArgs a) {
    constexpr int C8 = CG / 8, NK = (9 * CG + 63) / 64, MT = (CG + 15) / 16, NST = (MT + 1) / 2;
    constexpr int SMAX = gp_strips(CG, 2), TR = GP_ROWS + 1, TWMAX = 16 * SMAX + 1;
    __shared__ __attribute__((aligned(16))) int8_t ds[C8 * TR * TWMAX * 8];
    __shared__ __attribute__((aligned(16))) int8_t wsm[4 * NK * 32 * 16];
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
    const int a0 = band * GP_ROWS, s0 = seg * SMAX, b0 = 16 * s0;
    const int S = min(SMAX, ((nb + 15) >> 4) - s0);
    const int TW = 16 * S + 1;

    // the dy tile: rows a0 - 1 .., columns b0 - 1 .., zeros outside dy
    for (int e = threadIdx.x; e < TR * TW * C8; e += 256) {
        const int c8 = e % C8, px = e / C8;
        const int r = px / TW, c = px - r * TW;
        const int oy = a0 - 1 + r, ox = b0 - 1 + c;
        const bool ok = oy >= 0 && oy < a.ih && ox >= 0 && ox < a.iw;
        const v2i v = buf_load8(rd, ok ? (uint32_t)(((img * a.ih + oy) * a.iw + ox) * a.cp + grp * CG + 8 * c8) : OOB);
        *(v2i*)(ds + ((c8 * TR + r) * TW + c) * 8) = v;
    }
    const Gc2Quant z = gc2_quant<PASS>(a, gm);
    uint32_t m = 0;
    for (int st = 0; st < NST; ++st) {
        __syncthreads();
        gp_load_w<CG, true, false>(rw, grp, st, wsm);
        __syncthreads();
        gcp_dgrad2_class<CG, PASS, 0, 0>(a, ds, wsm, S, img, grp, st, a0, b0, na, z, m);
        gcp_dgrad2_class<CG, PASS, 0, 1>(a, ds, wsm, S, img, grp, st, a0, b0, na, z, m);
        gcp_dgrad2_class<CG, PASS, 1, 0>(a, ds, wsm, S, img, grp, st, a0, b0, na, z, m);
        gcp_dgrad2_class<CG, PASS, 1, 1>(a, ds, wsm, S, img, grp, st, a0, b0, na, z, m);
    }
    if (PASS == 1) gp_zero_pad(a, img, 2 * a0 - a.pad, 2 * GP_ROWS, 2 * b0 - a.pad, 32 * S);
    gc2_publish<PASS>(a, m, red);
}

// a.slab: [gridDim.x][C][9][CG]; gridDim.y = the groups, gridDim.z = the item quads of a group
template <int CG, int STRIDE>
__global__ void __launch_bounds__(256) gcp_wgrad_kernel(GcWgArgs a) {
    constexpr int MT = (CG + 15) / 16, CGP = 16 * MT, NTI = gp_wg_nti(MT), NTB = (MT + NTI - 1) / NTI;
    constexpr int SMAX = gp_strips(CG, STRIDE), XROWS = STRIDE * (GP_ROWS - 1) + 3;
    // pitches in bytes, for SMAX strips: a dy row, an x row of one plane (16 more: the kx shifts read on), a channel
    // of each (16 more: the pitch is an odd count of 16, a slot's 16 lanes read conflict-free)
    constexpr int DPMAX = 16 * SMAX, XPMAX = DPMAX + 16;
    __shared__ __attribute__((aligned(16))) int8_t dT[CGP * (GP_ROWS * DPMAX + 16)];
    __shared__ __attribute__((aligned(16))) int8_t xT[CGP * (XROWS * STRIDE * XPMAX + 16)];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4;
    const int grp = (int)blockIdx.y;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.xbytes), rd = make_rsrc(a.dy, a.dbytes);
    // this wave's item: output channels 16 to .., input channels 16 (ti0 + i) .., i < NTI, all 9 taps
    const int item = 4 * (int)blockIdx.z + wave;
    const int to = item / NTB, ti0 = (item - to * NTB) * NTI;
    const bool works = item < MT * NTB;

    v4i acc[NTI][3][3];
#pragma unroll
    for (int i = 0; i < NTI; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) acc[i][j][kx] = v4i{0, 0, 0, 0};

    const int strips_all = (a.ow + 15) >> 4;
    const int per_img = a.bands * a.segs;
    for (int unit = (int)blockIdx.x; unit < a.units; unit += (int)gridDim.x) {
        const int img = unit / per_img, tile = unit - img * per_img;
        const int band = tile / a.segs, seg = tile - band * a.segs;
        const int oy0 = band * GP_ROWS, s0 = seg * SMAX;
        const int S = min(SMAX, strips_all - s0);
        const int DP = 16 * S, XP = DP + 16;
        const int DCH = GP_ROWS * DP + 16, XCH = XROWS * STRIDE * XP + 16;
        __syncthreads();  // (the previous band's reads are over)
        // dy rows oy0 .. + 3, columns 16 s0 ..: four pixels x 8 channels -> 8 dwords of one channel's four pixels;
        // the channels past cg: zero rows
        for (int e = threadIdx.x; e < GP_ROWS * (DP / 4) * (CGP / 8); e += 256) {
            const int c8 = e % (CGP / 8), rest = e / (CGP / 8);
            const int pq = rest % (DP / 4), r = rest / (DP / 4);
            const int oy = oy0 + r;
            v2i v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int ox = 16 * s0 + 4 * pq + p;
                const bool ok = oy < a.oh && ox < a.ow && 8 * c8 < CG;
                v[p] = buf_load8(rd, ok ? (uint32_t)(((img * a.oh + oy) * a.ow + ox) * a.cp + grp * CG + 8 * c8) : OOB);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                int R[4];
                tr4(v[0][j], v[1][j], v[2][j], v[3][j], R);
#pragma unroll
                for (int b = 0; b < 4; ++b) *(int*)(dT + (8 * c8 + 4 * j + b) * DCH + r * DP + 4 * pq) = R[b];
            }
        }
        // x rows STRIDE oy0 - pad ..; pixel i of plane `par` is tile column STRIDE i + par at STRIDE 16 s0 - pad; at
        // stride 2 nothing past pixel 16 S is read for a product: zeros
        for (int e = threadIdx.x; e < XROWS * STRIDE * (XP / 4) * (CGP / 8); e += 256) {
            const int c8 = e % (CGP / 8), rest = e / (CGP / 8);
            const int pq = rest % (XP / 4), rp = rest / (XP / 4);
            const int r = rp / STRIDE, par = rp - r * STRIDE;
            const int iy = STRIDE * oy0 - a.pad + r;
            v2i v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int i = 4 * pq + p;
                const int ix = STRIDE * 16 * s0 - a.pad + STRIDE * i + par;
                const bool ok = (STRIDE == 1 || i <= 16 * S) && iy >= 0 && iy < a.h && ix >= 0 && ix < a.w && 8 * c8 < CG;
                v[p] = buf_load8(rx, ok ? (uint32_t)(((img * a.h + iy) * a.w + ix) * a.cp + grp * CG + 8 * c8) : OOB);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                int R[4];
                tr4(v[0][j], v[1][j], v[2][j], v[3][j], R);
#pragma unroll
                for (int b = 0; b < 4; ++b) *(int*)(xT + (8 * c8 + 4 * j + b) * XCH + rp * XP + 4 * pq) = R[b];
            }
        }
        __syncthreads();
        if (!works) continue;
        // MFMA k: K slot q = output row oy0 + q, strip s0 + k
        for (int k = 0; k < S; ++k) {
            const v4i fa = *(const v4i*)(dT + (16 * to + col) * DCH + q * DP + 16 * k);
#pragma unroll
            for (int i = 0; i < NTI; ++i) {
                if (ti0 + i >= MT) continue;  // (uniform: the last block of a row of tiles may be short)
                const int8_t* xc = xT + (16 * (ti0 + i) + col) * XCH + 16 * k;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int8_t* xr = xc + (STRIDE * q + j) * STRIDE * XP;  // (stride 2: the even plane; the odd one XP on)
                    const v4i lo = *(const v4i*)xr;
                    const int hi = *(const int*)(xr + 16);
                    const int d[5] = {lo[0], lo[1], lo[2], lo[3], hi};
                    v4i s1, s2;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        s1[e] = (int)__builtin_amdgcn_alignbyte((uint32_t)d[e + 1], (uint32_t)d[e], 1u);
                        s2[e] = (int)__builtin_amdgcn_alignbyte((uint32_t)d[e + 1], (uint32_t)d[e], 2u);
                    }
                    // stride 1: kx = the byte shift; stride 2: kx 0 / 1 the even / odd plane, kx 2 the even one pixel on
                    v4i f1 = s1, f2 = s2;
                    if constexpr (STRIDE == 2) {
                        f1 = *(const v4i*)(xr + XP);
                        f2 = s1;
                    }
                    acc[i][j][0] = mfma64(fa, lo, acc[i][j][0]);
                    acc[i][j][1] = mfma64(fa, f1, acc[i][j][1]);
                    acc[i][j][2] = mfma64(fa, f2, acc[i][j][2]);
                }
            }
        }
    }

    // acc[i][j][kx][e]: output channel 16 to + 4 q + e, input channel 16 (ti0 + i) + col of the group, tap (j, kx)
    if (!works) return;
    int32_t* sl = a.slab + (size_t)blockIdx.x * a.C * 9 * CG;
#pragma unroll
    for (int i = 0; i < NTI; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int o = 16 * to + 4 * q + e, ic = 16 * (ti0 + i) + col;
                    if (o < CG && ic < CG && ti0 + i < MT)
                        sl[((size_t)(grp * CG + o) * 9 + 3 * j + kx) * CG + ic] = acc[i][j][kx][e];
                }
}

int gp_segs(int cols, int cg, int stride) {
    const int s = gp_strips(cg, stride);
    return ((cols + 15) / 16 + s - 1) / s;
}

// the kernels of one width: [forward, input gradient at stride 1; forward, input gradient at stride 2][pass]
struct GpKernels {
    void (*act[4][2])(GcActArgs);
    void (*wgrad[2])(GcWgArgs);  // stride 1, 2
    int nz;                      // its gridDim.z
};
template <int CG>
const GpKernels* gp_kernels_of() {
    constexpr int MT = (CG + 15) / 16, NTI = gp_wg_nti(MT);
    static const GpKernels k = {{{gcp_act_kernel<CG, 1, false, 0>, gcp_act_kernel<CG, 1, false, 1>},
                                 {gcp_act_kernel<CG, 1, true, 0>, gcp_act_kernel<CG, 1, true, 1>},
                                 {gcp_act_kernel<CG, 2, false, 0>, gcp_act_kernel<CG, 2, false, 1>},
                                 {gcp_dgrad2_kernel<CG, 0>, gcp_dgrad2_kernel<CG, 1>}},
                                {gcp_wgrad_kernel<CG, 1>, gcp_wgrad_kernel<CG, 2>},
                                (MT * ((MT + NTI - 1) / NTI) + 3) / 4};
    return &k;
}
const GpKernels* gp_kernels(int cg) {
    switch (cg) {
        case 24: return gp_kernels_of<24>();
        case 40: return gp_kernels_of<40>();
        case 48: return gp_kernels_of<48>();
        case 56: return gp_kernels_of<56>();
        case 72: return gp_kernels_of<72>();
        case 80: return gp_kernels_of<80>();
        case 88: return gp_kernels_of<88>();
        case 96: return gp_kernels_of<96>();
        case 104: return gp_kernels_of<104>();
        case 112: return gp_kernels_of<112>();
        case 120: return gp_kernels_of<120>();
        case 128: return gp_kernels_of<128>();
        default: return nullptr;
    }
}

}  // namespace

// a workgroup a group; the weight gradient's z the width's item groups
const GcKernels& gc_packed() {
    static const GcKernels k = {
        gp_segs,
        [](int, int groups) { return (unsigned)groups; },
        [](int cg) { return (unsigned)gp_kernels(cg)->nz; },
        0,
        [](int cg, int stride, bool dgrad, int pass) { return gp_kernels(cg)->act[2 * (stride == 2) + (dgrad ? 1 : 0)][pass]; },
        [](int cg, int stride) { return gp_kernels(cg)->wgrad[stride == 2]; }};
    return k;
}

}  // namespace niti
