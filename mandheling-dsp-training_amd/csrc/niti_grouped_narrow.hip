// niti_grouped_narrow.hip -- grouped 3x3 conv layers at group widths 4 and 8 (the kernels and gc_narrow(); launched
// by niti_grouped_host.hip):
// groups = G >= 2, c_in = c_out = C = G * cg, C a multiple of 16, stride 1 or 2, one pad 0..2 on every side.
// What ResNeXt 32x4d's first two stages and the small RegNets run.  Semantics, the two-pass range protocol, the
// ActOut fields and the slab form are niti_grouped.hip's; the kernels are their own.
//
// A 16-row MFMA tile would hold 4 or 2 groups and be 3/4 or 1/2 structural zeros.  v_mfma_i32_4x4x4_16b_i8 is
// sixteen independent 4x4x4 int8 products an issue: lanes 4 b .. 4 b + 3 are block b; lane 4 b + i supplies row i
// of the block's A and column i of its B, each one dword of 4 K bytes; lane 4 b + j holds column j of the block's
// result, rows 0..3 in its four registers.
//
// Layouts.  Activations NHWC16 [n][h][w][C].  The weight, its int32 gradient and the gradient's slabs are
// [C][9][16], the OHWI16 form of a dense layer with c_in = cg (cip = 16), entries cg..15 zero: the update, combine,
// layout and snapshot launches take them as they take any dense layer's.
//
// gcn_act (forward; input gradient at stride 1: the same conv on dy, taps reversed, pad 2 - pad).  An instruction
// covers 64 consecutive channels x a quad of 4 output pixels of one row.  cg 4: block b is group b of the chunk,
// A = w[4 b + i][tap][0..3], B = x[pixel j][4 b .. 4 b + 3]: 9 MFMAs a quad.  cg 8: block b is (group b / 2, output
// half b % 2) and K runs over the group's two 4-channel chunks: 18 MFMAs, both halves reading the same 8 bytes of
// B.  Either way lane (b, j) ends with channels 4 b .. 4 b + 3 of pixel j: one dword of the int8 output.  For the
// input gradient A is the weight transposed within the group: tr4 once per wave, at load.  The 9 (18) A dwords of
// a lane stay in registers.  A workgroup takes (image, 64-channel chunk, 4 output rows, 32 columns); LDS:
//   xs [row][column][64 bytes]            stride 1: 6 rows x 34 columns; a quad's lanes read 256 contiguous bytes
//   xs [row][parity][column / 2][64 b.]   stride 2: 9 rows x 65 columns split by the parity of the tile column, so
//                                         tap kx of pixel j is plane kx & 1, column j + (kx >> 1): contiguous again
// zeros outside the image and past C (a partial last chunk: those blocks store nothing); a partial last quad
// computes its masked pixels and stores nothing.
//
// gcn_dgrad2 (input gradient at stride 2).  niti_grouped.hip's parity classes: Y = y + pad, X = x + pad, class
// (Y & 1, X & 1) admits the taps of that parity, dy((Y >> 1) - (ky >> 1), (X >> 1) - (kx >> 1)).  A quad is four dx
// pixels of one row and one column parity (x two apart, X >> 1 consecutive), so its reads of the dy tile
// [5 rows][33 columns][64 bytes] are contiguous.  One instantiation per class (4, 2, 2, 1 taps): no MFMA on an
// excluded tap, no zero-stuffed dy; a dx row or column no output reads finds only zeros in the tile.
//
// gcn_wgrad.  Per group and tap a cg x cg product over the pixels, K = 4 consecutive pixels of a row: A rows = dy
// channels, B columns = x channels, each the dword of one channel's four pixels.  A band's 4 dy rows and the x
// rows under them go to LDS channel-major through tr4, [channel][row][pixel] with channel pitches of an odd dword
// count (the 64 lanes read 64 channels at one pixel offset: conflict-free).  The kx shifts are v_alignbyte_b32 over
// an aligned dword and the next; at stride 2 x lies as two column-parity planes (kx 0 / 1 aligned reads, kx 2 the
// even plane one pixel on).  cg 4: acc[tap] (36 registers); cg 8: block b = (group b / 2, dy half b % 2) and one
// MFMA per x half, acc[tap][half] (72).  A wave accumulates over its share of the band's quads, the four waves
// reduce through LDS (over the tiles) in two rounds, and wave 0 writes the chunk's part of one slab, the zero
// padding included.  The slab count is a function of the shape alone.
#include <algorithm>

#include "niti_device.hpp"
#include "niti_grouped.hpp"
#include "niti_kernels.hpp"
#include "niti_sgd.hpp"

namespace niti {

namespace {

constexpr int GN_ROWS = 4;             // output rows of a band
constexpr int GN_COLS = 32;            // its columns: 8 quads
constexpr int GN_MIN_WORKGROUPS = 256;  // of the weight gradient: a chunk is 64 channels, so few chunks want more slabs

__device__ __forceinline__ int buf_load4(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return (int)__builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0);
}

__device__ __forceinline__ v4i mfma4(int a, int b, v4i c) { return __builtin_amdgcn_mfma_i32_4x4x4i8(a, b, c, 0, 0, 0); }

// This lane's (4 b + i) A dwords of weight tap `tap`, one per K chunk.  Forward: row = output channel c0 + 4 b + i,
// K = the group's input channels 4 kc ..  Input gradient (TR): row = input channel 4 b + i of the chunk, K = the
// group's output channels o0 ..: the 4 x 4 block w[o0 .. o0 + 3][tap][4 d .. 4 d + 3] transposed, the lane keeping
// row i.  Rows past C read zeros through the buffer bound.
template <int CG, bool TR>
__device__ __forceinline__ void gcn_load_a(const __amdgpu_buffer_rsrc_t rw, int c0, int tap, int (&A)[CG / 4]) {
    const int lane = threadIdx.x & 63, b = lane >> 2, i = lane & 3;
#pragma unroll
    for (int kc = 0; kc < CG / 4; ++kc) {
        if (!TR) {
            A[kc] = buf_load4(rw, (uint32_t)(((c0 + 4 * b + i) * 9 + tap) * 16 + 4 * kc));
        } else {
            const int o0 = c0 + (CG == 4 ? 4 * b : 8 * (b >> 1) + 4 * kc), d = CG == 4 ? 0 : (b & 1);
            int v[4], R[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = buf_load4(rw, (uint32_t)(((o0 + k) * 9 + tap) * 16 + 4 * d));
            tr4(v[0], v[1], v[2], v[3], R);
            A[kc] = i == 0 ? R[0] : i == 1 ? R[1] : i == 2 ? R[2] : R[3];
        }
    }
}

// one tap of a quad: p = the lane's pixel in the tile, at its block's K bytes (gcn_choff)
template <int CG>
__device__ __forceinline__ v4i gcn_mac(v4i acc, const int8_t* p, const int (&A)[CG / 4]) {
    if constexpr (CG == 4) {
        return mfma4(A[0], *(const int*)p, acc);
    } else {
        const int2 v = *(const int2*)p;  // the group's 8 channels: both K chunks
        return mfma4(A[1], v.y, mfma4(A[0], v.x, acc));
    }
}
template <int CG>
__device__ __forceinline__ int gcn_choff(int b) {
    return CG == 4 ? 4 * b : 8 * (b >> 1);
}

template <int CG, int STRIDE, bool DGRAD, int PASS>
__global__ void __launch_bounds__(256) gcn_act_kernel(GcActArgs a) {
    static_assert(!(STRIDE == 2 && DGRAD), "gcn_dgrad2_kernel");
    constexpr int KC = CG / 4;
    constexpr int TRMAX = STRIDE * (GN_ROWS - 1) + 3;             // tile rows
    constexpr int PW = STRIDE == 1 ? GN_COLS + 2 : GN_COLS + 1;  // columns of a plane
    constexpr int RP = STRIDE * PW * 64;                          // bytes of a tile row
    __shared__ __attribute__((aligned(16))) int8_t xs[TRMAX * RP];
    __shared__ uint32_t red[4];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane >> 2, j = lane & 3;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.xbytes), rw = make_rsrc(a.w, a.wbytes);
    uint32_t gm = 0;
    if (PASS == 1) gm = a.amax[lane * MAX_SLOT_STRIDE];

    const int c0 = 64 * (int)blockIdx.y;
    const int tiles = a.bands * a.segs;
    const int img = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - img * tiles;
    const int band = tile / a.segs, seg = tile - band * a.segs;
    const int oy0 = band * GN_ROWS, ox0 = seg * GN_COLS;
    const int nr = min(GN_ROWS, a.oh - oy0), nq = (min(GN_COLS, a.ow - ox0) + 3) >> 2;  // this tile's rows, quads
    const int tr = STRIDE * (nr - 1) + 3, tc = STRIDE * (4 * nq - 1) + 3;

    // the input tile: rows STRIDE oy0 - pad .., columns STRIDE ox0 - pad .., the chunk's 64 channels in 16-byte parts
    for (int e = threadIdx.x; e < tr * tc * 4; e += 256) {
        const int part = e & 3, px = e >> 2;
        const int r = px / tc, c = px - r * tc;
        const int iy = STRIDE * oy0 - a.pad + r, ix = STRIDE * ox0 - a.pad + c;
        const bool ok = iy >= 0 && iy < a.ih && ix >= 0 && ix < a.iw && c0 + 16 * part < a.C;
        const v4i v = buf_load16(rx, ok ? (uint32_t)(((img * a.ih + iy) * a.iw + ix) * a.C + c0 + 16 * part) : OOB);
        const int pc = STRIDE == 2 ? (c & 1) * PW + (c >> 1) : c;
        *(v4i*)(xs + r * RP + pc * 64 + 16 * part) = v;
    }
    int A[9][KC];
#pragma unroll
    for (int t = 0; t < 9; ++t) gcn_load_a<CG, DGRAD>(rw, c0, DGRAD ? 8 - t : t, A[t]);
    __syncthreads();

    const Gc2Quant z = gc2_quant<PASS>(a, gm);
    const bool chok = c0 + 4 * b < a.C;
    uint32_t m = 0;
    // a wave's units: the quads of the tile
    for (int u = wave; u < nr * nq; u += 4) {
        const int r = u / nq, q = u - r * nq;
        const int8_t* p = xs + STRIDE * r * RP + (4 * q + j) * 64 + gcn_choff<CG>(b);
        v4i acc{0, 0, 0, 0};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
                acc = gcn_mac<CG>(acc, p + ky * RP + (STRIDE == 1 ? kx : (kx & 1) * PW + (kx >> 1)) * 64, A[3 * ky + kx]);
        // acc[e]: pixel j of the quad, channel c0 + 4 b + e
        const int oy = oy0 + r, ox = ox0 + 4 * q + j;
        if (ox < a.ow && chok) gc2_emit<PASS>(a, acc, (((size_t)img * a.oh + oy) * a.ow + ox) * a.C + c0 + 4 * b, z, m);
    }
    gc2_publish<PASS>(a, m, red);
}

// One parity class (PY, PX) of the stride-2 input gradient over the wave's quads: dx pixels (2 Ay + PY - pad,
// 2 Bx + PX - pad) for Ay = a0 + r, Bx = b0 + 4 q + j; its taps (jy, jx) are ky = 2 jy or 1, kx = 2 jx or 1, reading
// dy(Ay - jy, Bx - jx) = tile (r + 1 - jy, 4 q + j + 1 - jx)
template <int CG, int PASS, int PY, int PX>
__device__ __forceinline__ void gcn_dgrad2_class(const GcActArgs& a, const int8_t* ds, const int (&A)[9][CG / 4], int nr,
                                                 int nq, int img, int c0, int a0, int b0, Gc2Quant z, uint32_t& m) {
    constexpr int TW = GN_COLS + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane >> 2, j = lane & 3;
    const bool chok = c0 + 4 * b < a.C;
    for (int u = wave; u < nr * nq; u += 4) {
        const int r = u / nq, q = u - r * nq;
        const int y = 2 * (a0 + r) + PY - a.pad, x = 2 * (b0 + 4 * q + j) + PX - a.pad;
        if (y < 0 || y >= a.oh) continue;  // (uniform)
        const int8_t* p = ds + ((r + 1) * TW + 4 * q + j + 1) * 64 + gcn_choff<CG>(b);
        v4i acc{0, 0, 0, 0};
#pragma unroll
        for (int jy = 0; jy < (PY ? 1 : 2); ++jy)
#pragma unroll
            for (int jx = 0; jx < (PX ? 1 : 2); ++jx)
                acc = gcn_mac<CG>(acc, p - (jy * TW + jx) * 64, A[3 * (PY ? 1 : 2 * jy) + (PX ? 1 : 2 * jx)]);
        if (x >= 0 && x < a.ow && chok)
            gc2_emit<PASS>(a, acc, (((size_t)img * a.oh + y) * a.ow + x) * a.C + c0 + 4 * b, z, m);
    }
}

// a: x = dy [n][ih][iw][C], out = dx [n][oh][ow][C], pad = the layer's; bands / segs over (Y >> 1, X >> 1)
template <int CG, int PASS>
__global__ void __launch_bounds__(256) gcn_dgrad2_kernel(GcActArgs a) {
    constexpr int TR = GN_ROWS + 1, TW = GN_COLS + 1;
    __shared__ __attribute__((aligned(16))) int8_t ds[TR * TW * 64];
    __shared__ uint32_t red[4];

    const int lane = threadIdx.x & 63;
    const __amdgpu_buffer_rsrc_t rd = make_rsrc(a.x, a.xbytes), rw = make_rsrc(a.w, a.wbytes);
    uint32_t gm = 0;
    if (PASS == 1) gm = a.amax[lane * MAX_SLOT_STRIDE];

    const int c0 = 64 * (int)blockIdx.y;
    const int tiles = a.bands * a.segs;
    const int img = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - img * tiles;
    const int band = tile / a.segs, seg = tile - band * a.segs;
    const int na = ((a.oh - 1 + a.pad) >> 1) + 1, nb = ((a.ow - 1 + a.pad) >> 1) + 1;
    const int a0 = band * GN_ROWS, b0 = seg * GN_COLS;
    const int nr = min(GN_ROWS, na - a0), nq = (min(GN_COLS, nb - b0) + 3) >> 2;
    const int tr = nr + 1, tc = 4 * nq + 1;

    // the dy tile: rows a0 - 1 .., columns b0 - 1 .., zeros outside dy
    for (int e = threadIdx.x; e < tr * tc * 4; e += 256) {
        const int part = e & 3, px = e >> 2;
        const int r = px / tc, c = px - r * tc;
        const int oy = a0 - 1 + r, ox = b0 - 1 + c;
        const bool ok = oy >= 0 && oy < a.ih && ox >= 0 && ox < a.iw && c0 + 16 * part < a.C;
        const v4i v = buf_load16(rd, ok ? (uint32_t)(((img * a.ih + oy) * a.iw + ox) * a.C + c0 + 16 * part) : OOB);
        *(v4i*)(ds + (r * TW + c) * 64 + 16 * part) = v;
    }
    int A[9][CG / 4];  // the taps as they lie; a class reads its own
#pragma unroll
    for (int t = 0; t < 9; ++t) gcn_load_a<CG, true>(rw, c0, t, A[t]);
    __syncthreads();

    const Gc2Quant z = gc2_quant<PASS>(a, gm);
    uint32_t m = 0;
    gcn_dgrad2_class<CG, PASS, 0, 0>(a, ds, A, nr, nq, img, c0, a0, b0, z, m);
    gcn_dgrad2_class<CG, PASS, 0, 1>(a, ds, A, nr, nq, img, c0, a0, b0, z, m);
    gcn_dgrad2_class<CG, PASS, 1, 0>(a, ds, A, nr, nq, img, c0, a0, b0, z, m);
    gcn_dgrad2_class<CG, PASS, 1, 1>(a, ds, A, nr, nq, img, c0, a0, b0, z, m);
    gc2_publish<PASS>(a, m, red);
}

// a.slab: [gridDim.x][C][9][16]
template <int CG, int STRIDE>
__global__ void __launch_bounds__(256) gcn_wgrad_kernel(GcWgArgs a) {
    constexpr int NH = CG / 4;                        // 4-channel parts of a group's x channels: MFMAs a tap
    constexpr int NACC = 9 * NH * 4;                  // accumulator registers
    constexpr int XR = STRIDE * (GN_ROWS - 1) + 3;    // x rows of a band
    constexpr int DP = GN_COLS, XP = GN_COLS + 4;     // bytes of a dy row, of an x row of one plane (one dword on)
    constexpr int DCH = GN_ROWS * DP + 4, XCH = XR * STRIDE * XP + 4;  // channel pitches
    static_assert((DCH / 4) % 2 == 1 && (XCH / 4) % 2 == 1, "odd dword counts: 64 channels at one offset, no conflict");
    constexpr int TILE = 64 * (DCH + XCH), RED = 2 * NACC * 64 * 4;
    __shared__ __attribute__((aligned(16))) int8_t sm[TILE > RED ? TILE : RED];
    int8_t* const dT = sm;
    int8_t* const xT = sm + 64 * DCH;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane >> 2, i = lane & 3;
    const int c0 = 64 * (int)blockIdx.y;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, a.xbytes), rd = make_rsrc(a.dy, a.dbytes);

    v4i acc[9][NH];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int h = 0; h < NH; ++h) acc[t][h] = v4i{0, 0, 0, 0};

    const int per_img = a.bands * a.segs;
    for (int unit = (int)blockIdx.x; unit < a.units; unit += (int)gridDim.x) {
        const int img = unit / per_img, tile = unit - img * per_img;
        const int band = tile / a.segs, seg = tile - band * a.segs;
        const int oy0 = band * GN_ROWS, ox0 = seg * GN_COLS;
        const int nr = min(GN_ROWS, a.oh - oy0), nq = (min(GN_COLS, a.ow - ox0) + 3) >> 2;
        __syncthreads();  // (the previous band's reads are over)
        // dy rows oy0 .., columns ox0 ..: four pixels x 16 channels -> 16 dwords of one channel's four pixels
        for (int e = threadIdx.x; e < nr * nq * 4; e += 256) {
            const int part = e & 3, rest = e >> 2;
            const int r = rest / nq, pq = rest - r * nq;
            v4i v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int ox = ox0 + 4 * pq + p;
                const bool ok = ox < a.ow && c0 + 16 * part < a.C;
                v[p] = buf_load16(rd, ok ? (uint32_t)(((img * a.oh + oy0 + r) * a.ow + ox) * a.C + c0 + 16 * part) : OOB);
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                int R[4];
                tr4(v[0][jj], v[1][jj], v[2][jj], v[3][jj], R);
#pragma unroll
                for (int bb = 0; bb < 4; ++bb) *(int*)(dT + (16 * part + 4 * jj + bb) * DCH + r * DP + 4 * pq) = R[bb];
            }
        }
        // x rows STRIDE oy0 - pad ..; pixel i of plane `par` is tile column STRIDE i + par at STRIDE ox0 - pad; one
        // quad past the band's: the kx shifts read it
        const int xr_n = STRIDE * (nr - 1) + 3;
        for (int e = threadIdx.x; e < xr_n * STRIDE * (nq + 1) * 4; e += 256) {
            const int part = e & 3, rest = e >> 2;
            const int rp = rest / (nq + 1), pq = rest - rp * (nq + 1);
            const int r = rp / STRIDE, par = rp - r * STRIDE;
            const int iy = STRIDE * oy0 - a.pad + r;
            v4i v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int ix = STRIDE * ox0 - a.pad + STRIDE * (4 * pq + p) + par;
                const bool ok = iy >= 0 && iy < a.h && ix >= 0 && ix < a.w && c0 + 16 * part < a.C;
                v[p] = buf_load16(rx, ok ? (uint32_t)(((img * a.h + iy) * a.w + ix) * a.C + c0 + 16 * part) : OOB);
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                int R[4];
                tr4(v[0][jj], v[1][jj], v[2][jj], v[3][jj], R);
#pragma unroll
                for (int bb = 0; bb < 4; ++bb) *(int*)(xT + (16 * part + 4 * jj + bb) * XCH + rp * XP + 4 * pq) = R[bb];
            }
        }
        __syncthreads();
        // a wave's quads: A = dy channel `lane`, B = x channel 4 b + i (cg 4) or 8 (b / 2) + 4 h + i (cg 8)
        for (int u = wave; u < nr * nq; u += 4) {
            const int r = u / nq, q = u - r * nq;
            const int fa = *(const int*)(dT + lane * DCH + r * DP + 4 * q);
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const int ch = CG == 4 ? lane : 8 * (b >> 1) + 4 * h + i;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const int8_t* xr = xT + ch * XCH + (STRIDE * r + ky) * STRIDE * XP + 4 * q;
                    const uint32_t lo = *(const uint32_t*)xr, hi = *(const uint32_t*)(xr + 4);
                    int f[3];
                    f[0] = (int)lo;
                    if (STRIDE == 1) {
                        f[1] = (int)__builtin_amdgcn_alignbyte(hi, lo, 1u);
                        f[2] = (int)__builtin_amdgcn_alignbyte(hi, lo, 2u);
                    } else {
                        f[1] = *(const int*)(xr + XP);
                        f[2] = (int)__builtin_amdgcn_alignbyte(hi, lo, 1u);
                    }
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) acc[3 * ky + kx][h] = mfma4(fa, f[kx], acc[3 * ky + kx][h]);
                }
            }
        }
    }

    // acc[tap][h][e] of lane (b, j = i): output channel c0 + 4 b + e, input channel 4 h + j of its group.  Waves 2, 3
    // into 0, 1, then 1 into 0.
    int32_t* const rb = (int32_t*)sm;
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        const int half = round == 0 ? 2 : 1;  // waves half .. 2 half - 1 give to waves 0 .. half - 1
        __syncthreads();
        if (wave >= half && wave < 2 * half)
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int h = 0; h < NH; ++h)
#pragma unroll
                    for (int e = 0; e < 4; ++e) rb[(((wave - half) * 9 + t) * NH + h) * 256 + e * 64 + lane] = acc[t][h][e];
        __syncthreads();
        if (wave < half)
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int h = 0; h < NH; ++h)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[t][h][e] += rb[((wave * 9 + t) * NH + h) * 256 + e * 64 + lane];
    }
    if (wave != 0 || c0 + 4 * b >= a.C) return;
    int32_t* sl = a.slab + ((size_t)blockIdx.x * a.C + c0 + 4 * b) * 9 * 16;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int h = 0; h < 4; ++h) sl[(e * 9 + t) * 16 + 4 * h + i] = h < NH ? acc[t][h < NH ? h : 0][e] : 0;
}

GcActKern gn_act_kernel(int cg, int stride, bool dgrad, int pass) {
    // [cg 4 / 8][forward, input gradient at stride 1; forward, input gradient at stride 2][pass]
    static const GcActKern tab[2][4][2] = {
        {{gcn_act_kernel<4, 1, false, 0>, gcn_act_kernel<4, 1, false, 1>},
         {gcn_act_kernel<4, 1, true, 0>, gcn_act_kernel<4, 1, true, 1>},
         {gcn_act_kernel<4, 2, false, 0>, gcn_act_kernel<4, 2, false, 1>},
         {gcn_dgrad2_kernel<4, 0>, gcn_dgrad2_kernel<4, 1>}},
        {{gcn_act_kernel<8, 1, false, 0>, gcn_act_kernel<8, 1, false, 1>},
         {gcn_act_kernel<8, 1, true, 0>, gcn_act_kernel<8, 1, true, 1>},
         {gcn_act_kernel<8, 2, false, 0>, gcn_act_kernel<8, 2, false, 1>},
         {gcn_dgrad2_kernel<8, 0>, gcn_dgrad2_kernel<8, 1>}}};
    return tab[cg == 8][2 * (stride == 2) + (dgrad ? 1 : 0)][pass];
}

GcWgKern gn_wgrad_kernel(int cg, int stride) {
    return stride == 2 ? (cg == 4 ? gcn_wgrad_kernel<4, 2> : gcn_wgrad_kernel<8, 2>)
                       : (cg == 4 ? gcn_wgrad_kernel<4, 1> : gcn_wgrad_kernel<8, 1>);
}

}  // namespace

// a workgroup a 64-channel chunk; the weight gradient wants enough workgroups (slabs x chunks) to cover the device
// where the units allow
const GcKernels& gc_narrow() {
    static const GcKernels k = {[](int cols, int, int) { return (cols + GN_COLS - 1) / GN_COLS; },
                                [](int C, int) { return (unsigned)((C + 63) / 64); },
                                [](int) { return 1u; },
                                GN_MIN_WORKGROUPS,
                                gn_act_kernel,
                                gn_wgrad_kernel};
    return k;
}

}  // namespace niti
