// niti_wgrad.hip -- weight gradient of NITI_GradientConv_Int8 (NITI_GradientConv_Int8.cpp:165-298;
// graph grad/NITI_Conv_Int8_Grad.cpp:124-191) for stride-1, pad-1 3x3 convolutions.
//
//   C[co][tap][ci] = sum over output pixels p of dy[p][co] * x[p + tap][ci]      (exact int32)
//
// Operand layout P16 ("pixel blocks"): an activation of P pixels (n, y, x) and Cp channels
// (Cp % 32 == 0, P % 16 == 0) is stored as [P/16][Cp][16]: 16 consecutive pixels of one channel
// are 16 contiguous bytes, and consecutive channels follow each other.  That is exactly the
// operand fragment of v_mfma_i32_32x32x32_i8 (lane l: column l & 31, k = 16 (l >> 5) + 0..15),
// so every lane loads its fragment straight from memory -- 16 bytes, 32 lanes reading 512
// contiguous bytes -- with no LDS staging, no transposed reads and no barrier in the K loop.
// (The NHWC16 kernels in niti_kernels.hip stage 32-byte channel segments of pixel rows through
// LDS; at 256 channels each 1 KiB LDS-DMA touched 32 cache lines and the loop ran at ~36 % of
// the MFMA rate.)
//
// A 16-pixel block is whole output rows (OW = 8: 2 rows, OW = 16: 1 row) or whole images
// (OW = 4: one 4x4 image, OW = 2: four 2x2 images).  The taps' B fragments come from the lane's
// window -- its block plus the rows above and below (OW 8 / 16, zero outside the image) -- by
// byte shifts in registers: a kx shift moves bytes inside a row (v_alignbit, zero filled at the
// row ends), a ky shift selects rows.
//
// Block: 32 output channels x 9 taps x 32 input channels (9 accumulator tiles, 36 KiB of int32).
// Its NW waves (one per SIMD) split the block's K range into contiguous runs of 32-pixel K groups
// (two blocks, one per half-wave) that cover whole images.  Loads -- dy, the x block and the x
// rows above / below it -- run D K groups ahead in registers (inline-asm loads with counted
// waits); every address moves through the uniform soffset, out-of-range reads return zeros, so
// the loop has no per-iteration branch and almost no address arithmetic.  The waves meet through LDS once
// at the end: each adds its tile into one row-major LDS tile, which leaves as 16-byte row chunks.
//
// Split K: the blocks of a split tile store their partial tiles (plain stores, C's layout) into
// per-split slabs, which splitk_reduce_linear sums into C with the max|C| of NITI_RangeEstimate.
// (An in-launch combine -- write-through partials, an arrival ticket, the last block summing --
// was measured: the publish and the latency-bound combine took ~15 us of a 26 us launch.  Round 3
// measured it again on the current kernel -- plain slab stores, agent-scope fences around a
// per-tile arrival word, the last split summing the others' slabs with 36 loads in flight: an 8x8 layer
// 26.1 us against 10.3 us + a 4.8 us reduce launch, and the autotuner then preferred the taps
// kernel for conv4; step 0.423 ms against 0.403 ms.)
#include <hip/hip_ext.h>

#include <string.h>

#include <algorithm>
#include <atomic>
#include <type_traits>
#include <vector>

#include "niti_device.hpp"
#include "niti_kernels.hpp"

namespace niti {

struct WgP16 {
    const int8_t* x;   // P16 [N*H*W/16][CIP][16]
    const int8_t* dy;  // P16 [N*OH*OW/16][COP][16]
    uint32_t xbytes, dybytes;
    int CIP, COP, c_out;
    int64_t ldc;       // C row pitch (elements): 9 * CIP
    int bpi;           // 16-pixel blocks per image (OW 8: 4, OW 16: 16)
    int kg_total, kg_per_split, kg_per_wave, splits;
    int tiles_ci, tiles;
    FastDiv fTiles, fTci;
    int32_t* C;
    uint32_t* amax;
    int32_t* slab;     // splits > 1: one C-shaped partial per split, slab_stride elements apart
    int64_t slab_stride;
    unsigned long long* span;
    unsigned long long* stamps;  // diagnostic builds
};

constexpr int P16_TILE = 9 * 32 * 32;  // int32 outputs per block tile
constexpr int P16_WAVES = 4;           // one wave per SIMD

// Diagnostic builds only (tools/wg_diag.sh): NITI_WG_STAMPS = 1 writes per-block s_memtime marks
// {start, loop entered, loop done, partials in LDS, output start, end, wall start, wall end} to the buffer armed by
// niti_diag_wgrad_stamps; NITI_WG_ABLATE skips a part (results wrong by design):
// 1 operand loads, 2 MFMA, 3 fragment shifts, 5 the output stores.
#ifndef NITI_WG_STAMPS
#define NITI_WG_STAMPS 0
#endif
#ifndef NITI_WG_ABLATE
#define NITI_WG_ABLATE 0
#endif
// NITI_WG_ATOMIC_OUT = 1 (diagnostic timing): split partials atomically added into C instead of slabs
// ring depth (K groups in flight) of the 8x8-image kernel; diagnostic builds vary it (the K loop
// ran the same 358 cycles per K group at depth 4, 6 and 8 on conv4; deeper rings only lengthen
// the prologue)
#ifndef NITI_WG_D8
#define NITI_WG_D8 4
#endif
#ifndef NITI_WG_D4  // ... and of the 4x4 / 2x2-image kernels
#define NITI_WG_D4 4
#endif
// merge of the 4 waves' partial tiles: 1 = register-owned quarters exchanged through LDS,
// 0 = ds_add into one LDS tile (diagnostic builds A/B them)
#ifndef NITI_WG_MERGE
#define NITI_WG_MERGE 1
#endif
#ifndef NITI_WG_NT_OUT
#define NITI_WG_NT_OUT 1
#endif
// NITI_WG_SWAP = 1: the MFMAs compute the transposed tile (x taps as A, dy taps as B), so after the
// merge a lane holds 4 consecutive ci of one co and the slab stores are 16 bytes wide
#ifndef NITI_WG_SWAP
#define NITI_WG_SWAP 1
#endif
#ifndef NITI_WG_ATOMIC_OUT
#define NITI_WG_ATOMIC_OUT 0
#endif
// (Measured and dropped, round 2: zeroing the accumulators ahead of the first ring wait, and a
// sched_group_barrier interleave of one MFMA with 2-3 VALU per K group -- 321 vs 342 cycles per K
// group, but the block end moved < 1 %: the merge and the output dominate the tail.)
// per-wave stamps (diagnostic): wave start and K-loop end after the 8 block stamps
#define WG_WSTAMP(k)                                                                                       \
    do {                                                                                                   \
        if (NITI_WG_STAMPS && g.stamps != nullptr && (threadIdx.x & 63) == 0)                              \
            g.stamps[gridDim.x * 8 + (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + (k)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#define WG_STAMP(k)                                                                            \
    do {                                                                                       \
        if (NITI_WG_STAMPS && g.stamps != nullptr && threadIdx.x == 0) {                        \
            g.stamps[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memtime();                     \
            if ((k) == 0 || (k) == 5)                                                          \
                g.stamps[blockIdx.x * 8 + 6 + ((k) == 5)] = __builtin_amdgcn_s_memrealtime();  \
        }                                                                                      \
    } while (0)

__device__ __forceinline__ int ab(int hi, int lo, int s) {
    return (int)__builtin_amdgcn_alignbit((uint32_t)hi, (uint32_t)lo, (uint32_t)s);
}

// v_perm_b32 byte selectors for a 2x2 image in one dword (byte 2 oy + ox); 0x0c reads a zero byte
template <int DY, int DX>
constexpr uint32_t perm2x2() {  // out(oy, ox) = in(oy + DY, ox + DX)
    uint32_t s = 0;
    for (int i = 0; i < 4; ++i) {
        const int iy = (i >> 1) + DY, ix = (i & 1) + DX;
        const uint32_t b = (iy >= 0 && iy < 2 && ix >= 0 && ix < 2) ? (uint32_t)(2 * iy + ix) : 0x0cu;
        s |= b << (8 * i);
    }
    return s;
}

// The taps.  C[co][ky][kx][ci] = sum over (oy, ox) of dy[oy][ox - kx + 1][co] * x[oy + ky - 1][ox][ci]
// (substituting ox -> ox - kx + 1; dy and x read as zero outside the image): the kx shift moves
// along dy's rows, the ky shift selects x's rows.  A lane's dy fragment is 16 pixels (OW 8: two
// rows, OW 16: one row, OW 4: one 4x4 image, OW 2: four 2x2 images, one dword each); its x
// window adds the row above and below (OW 8 / 16).
//
// A operand for tap column kx: dy shifted by kx - 1 pixels inside each row, zero filled.
template <int OW, int KX>
__device__ __forceinline__ v4i dy_tap(v4i d) {
    if constexpr (KX == 1) {
        return d;
    } else if constexpr (OW == 8) {  // two 8-byte rows
        if constexpr (KX == 0)
            return v4i{ab(d[1], d[0], 8), (int)((uint32_t)d[1] >> 8), ab(d[3], d[2], 8), (int)((uint32_t)d[3] >> 8)};
        else
            return v4i{(int)((uint32_t)d[0] << 8), ab(d[1], d[0], 24), (int)((uint32_t)d[2] << 8), ab(d[3], d[2], 24)};
    } else if constexpr (OW == 16) {  // one 16-byte row
        if constexpr (KX == 0)
            return v4i{ab(d[1], d[0], 8), ab(d[2], d[1], 8), ab(d[3], d[2], 8), (int)((uint32_t)d[3] >> 8)};
        else
            return v4i{(int)((uint32_t)d[0] << 8), ab(d[1], d[0], 24), ab(d[2], d[1], 24), ab(d[3], d[2], 24)};
    } else if constexpr (OW == 4) {  // four 4-byte rows
        v4i r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = KX == 0 ? (int)((uint32_t)d[i] >> 8) : (int)((uint32_t)d[i] << 8);
        return r;
    } else {  // four 2x2 images
        constexpr uint32_t sel = perm2x2<0, 1 - KX>();
        v4i r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = (int)__builtin_amdgcn_perm((uint32_t)d[i], (uint32_t)d[i], sel);
        return r;
    }
}

// B operand for tap row ky from the lane's block and the rows above / below it (OW 8: 8-byte
// rows in .xy, OW 16: whole 16-byte rows; OW 4 / 2: the block is whole images)
template <int OW, int KY>
__device__ __forceinline__ v4i x_tap(const v4i& up, const v4i& x, const v4i& dn) {
    if constexpr (KY == 1) {
        return x;
    } else if constexpr (OW == 8) {
        return KY == 0 ? v4i{up[0], up[1], x[0], x[1]} : v4i{x[2], x[3], dn[0], dn[1]};
    } else if constexpr (OW == 16) {
        return KY == 0 ? up : dn;
    } else if constexpr (OW == 4) {
        return KY == 0 ? v4i{0, x[0], x[1], x[2]} : v4i{x[1], x[2], x[3], 0};
    } else {
        constexpr uint32_t sel = perm2x2<KY - 1, 0>();
        v4i r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = (int)__builtin_amdgcn_perm((uint32_t)x[i], (uint32_t)x[i], sel);
        return r;
    }
}

__device__ __forceinline__ v2i asm_load8(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    v2i v;
    asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "=v"(v) : "v"(voff), "s"(r), "s"(soff));
    return v;
}
__device__ __forceinline__ v4i asm_load16(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    v4i v;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(v) : "v"(voff), "s"(r), "s"(soff));
    return v;
}

// LDS of a block: merge 0: one row-major tile every wave ds_adds into; merge 1: quarter slots
// [src wave][dst wave][tap][lane] (16 x 9 KiB, the 4 diagonal slots unused); plus the block-max scratch
constexpr int P16_SMEM = (NITI_WG_MERGE ? 4 * P16_TILE * 4 : P16_TILE * 4) + 64;

// One item: tile `tile` of the layer over the K groups [kg_begin, kg_end) (whole images), each wave a
// contiguous run of kg_per_wave of them.  slab < 0: the item is the tile's whole K range -- it goes
// to C and its block max into amax; else a partial tile into slab `slab`.  The per-layer kernel
// runs one item per block, wgrad_p16_many_kernel a list of them; the caller synchronises the
// block before the next item touches lds4 again.
//
// QUAD (wgrad_p16_many_kernel, short-K unsplit layers): the item is quad_n <= NW consecutive tiles
// from `tile` on, one per wave, each wave running the whole K range [kg_begin, kg_end) of its own
// tile -- no cross-wave sum.  A wave beyond quad_n runs as a wave without K groups does: dy pushed
// out of range, no stores, no contribution to the range.
template <int OW, int NW, int D, bool QUAD = false>
__device__ __forceinline__ void wgrad_p16_item(const WgP16& g, int tile, int slab, int kg_begin, int kg_end,
                                               int kg_per_wave, v4i* lds4, int quad_n = 0) {
    static_assert(D >= 2 && D % 2 == 0, "the next K group's window must be resident; operand buffers alternate");
    // the block's tile, row-major [co 32][tap 9][ci 32] int32 (every wave adds its partial into it),
    // plus the block-max scratch
    constexpr int SMEM = P16_SMEM;
    // typed as 16-byte vectors: the exchange stores / loads go through lds4 itself (byte-array
    // storage accessed as v4i is an aliasing violation the optimiser is free to act on)
    int8_t* smem = (int8_t*)lds4;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    WG_STAMP(0);
    WG_WSTAMP(0);
    if constexpr (QUAD) tile += wid;  // (a wave beyond quad_n: any tile, it only reads)
    const int tco = (int)fdiv(g.fTci, (uint32_t)tile), tci = tile - tco * g.tiles_ci;
    const int co0 = tco * 32, ci0 = tci * 32;
    // the wave's K groups: a contiguous run [kb, kb + n_w) of the item's range, whole images
    // (the range and kg_per_wave are multiples of the K groups per image); QUAD: the whole range
    const int kb = QUAD ? kg_begin : kg_begin + wid * kg_per_wave;
    const int n_w = QUAD ? (wid < quad_n ? kg_end - kg_begin : 0) : max(0, min(kg_end, kb + kg_per_wave) - kb);

    const __amdgpu_buffer_rsrc_t rX = make_rsrc(g.x, g.xbytes);
    const __amdgpu_buffer_rsrc_t rD = make_rsrc(g.dy, g.dybytes);
    const int h = lane >> 5, c = lane & 31;
    // byte offsets of the lane's fragment in K group kg: block b = 2 kg + h
    const uint32_t xrow = (uint32_t)g.CIP * 16u, drow = (uint32_t)g.COP * 16u;
    const uint32_t lx = (uint32_t)h * xrow + (uint32_t)(ci0 + c) * 16u;
    const uint32_t ld = (uint32_t)h * drow + (uint32_t)(co0 + c) * 16u;
    // The ring loads are inline asm, so their vmcnt is ours (hipcc's waitcnt insertion drained the
    // ring at the loop head).  A lane's voffset is fixed (channel, half-wave, image position of
    // the K group); the K group moves the uniform soffset.  The range check covers voffset +
    // soffset (measured, tools/probes/soffset_probe.hip), so look-ahead past the tensor reads
    // zeros, and dy past the wave's run is pushed out of range through its soffset.
    constexpr uint32_t OOBS = 0x80000000u;
    const uint32_t ci16 = (uint32_t)(ci0 + c) * 16u;

    v16i acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0;
    int32_t* tile_lds = (int32_t*)smem;
    if (!NITI_WG_MERGE)
        for (int e = tid; e < P16_TILE / 4; e += NW * 64) ((v4i*)tile_lds)[e] = v4i{0, 0, 0, 0};

    // OW 8 / 16: the rows above / below the lane's block are loaded as well (OW 8: the 8-byte row
    // of the block before / after, OW 16: the whole block).  Runs are whole images (KPI K groups
    // each), so the image position of every unrolled step is known: the first K group of an image
    // has no row above its first block, the last none below its second block.
    //   above, first K group of an image: half 1 <- block 2 kg (its own K group), half 0 zero
    //   above, otherwise: block 2 kg + h - 1 (soffset one block back)
    //   below: block 2 kg + h + 1; the last K group's half 1 zero
    constexpr bool NB = OW == 8 || OW == 16;
    constexpr int KPI = OW == 8 ? 2 : OW == 16 ? 8 : 1;  // K groups per image
    constexpr uint32_t UPOFF = OW == 8 ? 8u : 0u;       // the block above's last row
    constexpr int L = NB ? 4 : 2;                        // loads per K group
    static_assert(D % KPI == 0, "unrolled steps cover whole images");
    const uint32_t vup_first = h ? ci16 + UPOFF : OOB, vup = lx + UPOFF;
    const uint32_t vdn = lx + xrow, vdn_last = h ? OOB : lx + xrow;
    // ring slot: dy, the x block, the rows above / below (OW 8: one 8-byte row each)
    typedef typename std::conditional<OW == 8, v2i, v4i>::type Row;
    struct Ring {
        v4i d, x;
        Row up, dn;
    };
    Ring ring[D];
    auto issue = [&](Ring& r, auto u_c, int j) {
        constexpr int U = decltype(u_c)::value;
        const uint32_t sx = (uint32_t)(kb + j) * 2u * xrow;
        const uint32_t sd = j < n_w ? (uint32_t)(kb + j) * 2u * drow : OOBS;
        if (NITI_WG_ABLATE == 1) return;
        r.d = asm_load16(rD, ld, sd);
        r.x = asm_load16(rX, lx, sx);
        if constexpr (NB) {
            constexpr bool first = U % KPI == 0, last = U % KPI == KPI - 1;
            if constexpr (OW == 8) {
                r.up = first ? asm_load8(rX, vup_first, sx) : asm_load8(rX, vup, sx - xrow);
                r.dn = asm_load8(rX, last ? vdn_last : vdn, sx);
            } else {
                r.up = first ? asm_load16(rX, vup_first, sx) : asm_load16(rX, vup, sx - xrow);
                r.dn = asm_load16(rX, last ? vdn_last : vdn, sx);
            }
        }
    };
    [&]<int... U>(std::integer_sequence<int, U...>) {
        ((ring[U] = Ring{}, issue(ring[U], std::integral_constant<int, U>(), U)), ...);
    }(std::make_integer_sequence<int, D>());
    WG_STAMP(1);
    // Software pipeline: the tap operands of K group j + 1 (dy shifted for kx = 0 / 2, x rows for
    // ky = 0 / 2; kx = ky = 1 are the ring registers themselves) are built while K group j's nine
    // MFMAs run, so the VALU work fills MFMA gaps instead of stalling the pipe at every K group.
    struct Ops {
        v4i a0, a2, b0, b2;
    };
    Ops ops[2];
    auto prep = [&](Ring& r, Ops& o) {
        reg_fence(r.d);
        reg_fence(r.x);
        if constexpr (NB) {
            reg_fence(r.up);
            reg_fence(r.dn);
        }
        v4i up{0, 0, 0, 0}, dn{0, 0, 0, 0};
        if constexpr (OW == 8) {
            up = v4i{r.up[0], r.up[1], 0, 0};
            dn = v4i{r.dn[0], r.dn[1], 0, 0};
        } else if constexpr (OW == 16) {
            up = r.up;
            dn = r.dn;
        }
        if constexpr (NITI_WG_ABLATE == 3) {
            o.a0 = o.a2 = r.d;
            o.b0 = o.b2 = r.x;
        } else {
            o.a0 = dy_tap<OW, 0>(r.d);
            o.a2 = dy_tap<OW, 2>(r.d);
            o.b0 = x_tap<OW, 0>(up, r.x, dn);
            o.b2 = x_tap<OW, 2>(up, r.x, dn);
        }
    };
    wait_vmcnt<L * (D - 1)>();  // K group 0 has landed
    prep(ring[0], ops[0]);
    auto step = [&](auto u_c, int j0) {
        constexpr int u = decltype(u_c)::value, un = (u + 1) % D;
        // K group j + 1 has landed (j + 2 .. j + D - 1 may still be in flight): its operands
        wait_vmcnt<L * (D - 2)>();
        prep(ring[un], ops[(u + 1) & 1]);
        const Ops& o = ops[u & 1];
        const v4i A[3] = {o.a0, ring[u].d, o.a2};
        const v4i B[3] = {o.b0, ring[u].x, o.b2};
        [&]<int... T>(std::integer_sequence<int, T...>) {
            (([&] {
                 constexpr int KY = T / 3, KX = T % 3;
                 if constexpr (NITI_WG_ABLATE == 2)
                     acc[T][0] += A[KX][0] ^ B[KY][1];
                 else if constexpr (NITI_WG_MERGE && NITI_WG_SWAP)  // C^T: a lane holds one co, rows = ci
                     acc[T] = __builtin_amdgcn_mfma_i32_32x32x32_i8(B[KY], A[KX], acc[T], 0, 0, 0);
                 else
                     acc[T] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[KX], B[KY], acc[T], 0, 0, 0);
             }()),
             ...);
        }(std::make_integer_sequence<int, 9>());
        // slot u is free again: K group j + D
        issue(ring[u], u_c, j0 + u + D);
    };
    for (int j0 = 0; j0 < n_w; j0 += D) {
        [&]<int... U>(std::integer_sequence<int, U...>) {
            (step(std::integral_constant<int, U>(), j0), ...);
        }(std::make_integer_sequence<int, D>());
    }
    // The last D look-ahead loads (and all of them for a wave without K groups) are never consumed:
    // to hipcc their destination registers are dead at once, and it may hand them to other values
    // while the loads are still in flight.  Drain, then touch every ring register, so none of them
    // is reused before its data has landed.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int u = 0; u < D; ++u) {
        reg_fence(ring[u].d);
        reg_fence(ring[u].x);
        if constexpr (NB) {
            reg_fence(ring[u].up);
            reg_fence(ring[u].dn);
        }
    }
    WG_STAMP(2);
    WG_WSTAMP(1);

    constexpr int THREADS = NW * 64;
    const bool partial = slab >= 0;
    int32_t* dst = partial ? g.slab + (int64_t)slab * g.slab_stride : g.C;
    uint32_t lmax = 0;
    uint32_t* red = (uint32_t*)(smem + SMEM - 64);
    if constexpr (QUAD) {
        // The wave's tile is whole: nothing to sum.  Stores straight from the accumulator layout
        // cover 32 bytes per row per instruction (round 2: output 9.5k cycles against 2.9k), so the
        // wave turns its tile through its own quarter of the merge buffer -- the slots
        // [wid][q][tap] and the swizzle of the merged form below -- and reads it back in four
        // passes of 8 rows (co = 8 p + r), each the merged form's 9 ds_read_b128 and 9 stores of
        // 8 rows x 128 bytes.  Only this wave touches its quarter and a wave's LDS accesses
        // execute in order, so no workgroup barrier: a wave-scope fence keeps the compiler's order.
        static_assert(NITI_WG_MERGE && NITI_WG_SWAP && NW == 4, "the transposed tile's slots, a quarter per wave");
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int t = 0; t < 9; ++t)
                lds4[((wid * 4 + q) * 9 + t) * 64 + (lane ^ (2 * q + (lane >> 5) + 8 * (q & 1)))] =
                    v4i{acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]};
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        WG_STAMP(3);
        WG_STAMP(4);
        const int r = lane >> 3, c = lane & 7, q = c >> 1;
        const bool live = wid < quad_n;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int co = 8 * p + r;
            const int pos = (co + 32 * (c & 1)) ^ (c + 8 * ((c >> 1) & 1));
            v4i sum[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) sum[t] = lds4[((wid * 4 + q) * 9 + t) * 64 + pos];
            if (live && co0 + co < g.c_out && NITI_WG_ABLATE != 5) {
                int32_t* o = dst + (int64_t)(co0 + co) * g.ldc + ci0 + 4 * c;
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    __builtin_nontemporal_store(sum[t], (v4i*)(o + t * g.CIP));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t u = uabs32(sum[t][j]);
                        lmax = lmax > u ? lmax : u;
                    }
                }
            }
        }
    } else if constexpr (NITI_WG_MERGE) {
        static_assert(NW == 4, "one accumulator row quarter per wave");
        if constexpr (NITI_WG_SWAP) {
            // The tile is C^T: lane (co = lane & 31, h = lane >> 5) holds, in accumulator registers
            // 4q..4q+3, the 16 bytes ci 8q + 4h + 0..3 of row co.  Wave w owns rows co 8w..8w+7:
            // every wave writes its whole partial tile to LDS, slot [src wave][q][tap], and wave w's
            // lane (r = lane >> 3, c = lane & 7) sums the four waves' 16 bytes ci 4c..4c+3 of row
            // 8w + r -- so each store instruction covers 8 rows x 128 contiguous bytes (9 16-byte
            // stores per wave; the tail is store-issue bound, 36 dword stores took 3x as long).
            // The lane position inside a slot is XOR-swizzled by s = (2q + h) + 8 (q & 1): a
            // ds_write_b128 group (8 consecutive lanes, fixed q and h) stays a permutation of one
            // 128-byte run, and the 16 lanes of each ds_read_b128 group ({0-3,12-15,20-27}, ...)
            // land on 16 different 16-byte bank slots (XOR by 2q + h alone leaves them 2-way).
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int t = 0; t < 9; ++t)
                    lds4[((wid * 4 + q) * 9 + t) * 64 + (lane ^ (2 * q + (lane >> 5) + 8 * (q & 1)))] =
                        v4i{acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]};
            __syncthreads();  // every partial tile is in LDS (waits for the slowest wave's K loop)
            WG_STAMP(3);
            const int r = lane >> 3, c = lane & 7, co = 8 * wid + r;
            const int pos = (co + 32 * (c & 1)) ^ (c + 8 * ((c >> 1) & 1)), q = c >> 1;
            v4i sum[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) sum[t] = lds4[((0 * 4 + q) * 9 + t) * 64 + pos];
#pragma unroll
            for (int w = 1; w < 4; ++w)
#pragma unroll
                for (int t = 0; t < 9; ++t) sum[t] += lds4[((w * 4 + q) * 9 + t) * 64 + pos];
            WG_STAMP(4);
            if (co0 + co < g.c_out && NITI_WG_ABLATE != 5) {
                int32_t* o = dst + (int64_t)(co0 + co) * g.ldc + ci0 + 4 * c;
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    __builtin_nontemporal_store(sum[t], (v4i*)(o + t * g.CIP));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t u = uabs32(sum[t][j]);
                        lmax = lmax > u ? lmax : u;
                    }
                }
            }
        } else {
        // The waves meet through 16-byte lane-linear LDS writes: quarter q of a wave's partial tile
        // is accumulator registers 4q..4q+3 (rows 8q + 0..3 + 4h); wave w owns quarter w, sends
        // the other three to their owners, adds the three it receives to its own and stores those
        // rows straight from registers -- no atomics, no row-major staging tile.
        // slot [src wave][dst wave][tap][lane]: a wave writes only the three quarters it does
        // not own and keeps its own quarter in registers
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q != wid) {
#pragma unroll
                for (int t = 0; t < 9; ++t)
                    lds4[((wid * 4 + q) * 9 + t) * 64 + lane] =
                        v4i{acc[t][4 * q], acc[t][4 * q + 1], acc[t][4 * q + 2], acc[t][4 * q + 3]};
            }
        v4i sum[9];
        switch (wid) {  // the own quarter, registers 4w..4w+3 (static indices per case)
#define NITI_OWN(W)                                                                                          \
    case W:                                                                                                  \
        for (int t = 0; t < 9; ++t) sum[t] = v4i{acc[t][4 * W], acc[t][4 * W + 1], acc[t][4 * W + 2], acc[t][4 * W + 3]}; \
        break;
            NITI_OWN(0)
            NITI_OWN(1)
            NITI_OWN(2)
            default:
                NITI_OWN(3)
#undef NITI_OWN
        }
        __syncthreads();  // every quarter is in LDS (waits for the slowest wave's K loop)
        WG_STAMP(3);
#pragma unroll
        for (int k = 1; k < 4; ++k) {  // the other three waves, no branches: all 27 reads in flight
            const int w = (wid + k) & 3;
#pragma unroll
            for (int t = 0; t < 9; ++t) sum[t] += lds4[((w * 4 + wid) * 9 + t) * 64 + lane];
        }
        WG_STAMP(4);
        // rows 8w + j + 4h, column lane & 31: 128-byte runs per half-wave and register
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = 8 * wid + j + 4 * (lane >> 5);
            if (co0 + row < g.c_out && NITI_WG_ABLATE != 5) {
                int32_t* o = dst + (int64_t)(co0 + row) * g.ldc + ci0 + (lane & 31);
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int32_t v = sum[t][j];
                    __builtin_nontemporal_store(v, o + t * g.CIP);
                    const uint32_t u = uabs32(v);
                    lmax = lmax > u ? lmax : u;
                }
            }
        }
        }
    } else {
    // the waves meet: each adds its partial tile into the zeroed LDS tile (ds_add, the two
    // half-waves on separate 128-byte rows); then every thread stores 16-byte row chunks
    __syncthreads();  // the zeroed tile (the K loop has no barrier; this one waits for the slowest wave)
    WG_STAMP(3);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
            __hip_atomic_fetch_add(tile_lds + (row * 9 + t) * 32 + (lane & 31), acc[t][i], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    __syncthreads();
    WG_STAMP(4);

    // ---- output: C[co][tap][ci] (S = 1), or this split's C-shaped partial (reduced by
    // splitk_reduce_linear); chunk c = (row, tap, 4 columns)
    for (int c = tid; c < P16_TILE / 4; c += THREADS) {
        const int row = c / 72, rem = c - row * 72, t = rem >> 3, c4 = rem & 7;
        const v4i v = ((const v4i*)tile_lds)[c];
        if (co0 + row < g.c_out && NITI_WG_ABLATE != 5) {
            if (NITI_WG_ATOMIC_OUT && partial) {  // diagnostic: split-K partials added into C
                int32_t* q = g.C + (int64_t)(co0 + row) * g.ldc + t * g.CIP + ci0 + 4 * c4;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    __hip_atomic_fetch_add(q + e, v[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else if (NITI_WG_NT_OUT) {  // streaming stores: the partials leave L2 during the kernel
                __builtin_nontemporal_store(v, (v4i*)(dst + (int64_t)(co0 + row) * g.ldc + t * g.CIP + ci0 + 4 * c4));
            } else {
                *(v4i*)(dst + (int64_t)(co0 + row) * g.ldc + t * g.CIP + ci0 + 4 * c4) = v;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t u = uabs32(v[e]);
                lmax = lmax > u ? lmax : u;
            }
        }
    }
    }
    if (!partial && g.amax != nullptr) {
        lmax = wave_max(lmax);
        if (lane == 0) red[wid] = lmax;
        __syncthreads();
        if (tid == 0) {
            uint32_t m = red[0];
            for (int w = 1; w < NW; ++w) m = m > red[w] ? m : red[w];
            publish_max(g.amax, m);
        }
    }
    if (NITI_WG_STAMPS) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        WG_STAMP(5);
    }
}

// one layer per launch: block = (split, tile), one item
template <int OW, int NW, int D>
__global__ void __launch_bounds__(NW * 64) wgrad_p16_kernel(WgP16 g) {
    __shared__ v4i lds4[P16_SMEM / 16];
    const unsigned long long span_t0 = span_begin(g.span);
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int split = (int)fdiv(g.fTiles, (uint32_t)logical);
    const int tile = logical - split * g.tiles;
    const int kg_begin = split * g.kg_per_split;
    const int kg_end = min(g.kg_total, kg_begin + g.kg_per_split);
    wgrad_p16_item<OW, NW, D>(g, tile, g.splits > 1 ? split : -1, kg_begin, kg_end, g.kg_per_wave, lds4);
    span_end(g.span, span_t0);
}

// Every P16 weight gradient of a step as one persistent launch: block b runs the items
// [starts[b], starts[b + 1]) of a table the host packed (wgrad_p16_many_build), one after another.
// An item names its layer's descriptor, a tile and a K range; the block reads them through uniform
// addresses, dispatches on the layer's image width and synchronises before the next item reuses
// the LDS merge buffer.  No ticket, no atomics but the range word of unsplit layers.
struct WgP16Desc {
    WgP16 g;
    int ow, pad;
};
// quad > 0: the quad form -- `quad` (1..4) consecutive tiles from `tile` on, one per wave, each over
// the whole range [kg_begin, kg_end) (slab -1: quads are cut from unsplit layers only)
struct WgP16Item {
    int job, tile, slab, kg_begin, kg_end, kg_per_wave, quad, pad1;
};
// the quad form needs the transposed tile's LDS slots (diagnostic builds may turn them off)
constexpr bool P16_QUAD_OK = NITI_WG_MERGE && NITI_WG_SWAP;
template <int NW>
__global__ void __launch_bounds__(NW * 64) wgrad_p16_many_kernel(const WgP16Desc* __restrict__ descs,
                                                                  const int* __restrict__ starts,
                                                                  const WgP16Item* __restrict__ items) {
    __shared__ v4i lds4[P16_SMEM / 16];
    const int i0 = starts[blockIdx.x], i1 = starts[blockIdx.x + 1];
    for (int i = i0; i < i1; ++i) {
        const int job = __builtin_amdgcn_readfirstlane(items[i].job);
        const int tile = __builtin_amdgcn_readfirstlane(items[i].tile);
        const int slab = __builtin_amdgcn_readfirstlane(items[i].slab);
        const int kg_begin = __builtin_amdgcn_readfirstlane(items[i].kg_begin);
        const int kg_end = __builtin_amdgcn_readfirstlane(items[i].kg_end);
        const int kpw = __builtin_amdgcn_readfirstlane(items[i].kg_per_wave);
        const int quad = __builtin_amdgcn_readfirstlane(items[i].quad);
        const WgP16 g = descs[job].g;
        const int ow = __builtin_amdgcn_readfirstlane(descs[job].ow);
        if constexpr (P16_QUAD_OK) {
            if (quad > 0) {  // (the schedule cuts quads from 2x2 / 4x4 layers only: short K is small maps)
                if (ow == 4)
                    wgrad_p16_item<4, NW, NITI_WG_D4, true>(g, tile, -1, kg_begin, kg_end, kpw, lds4, quad);
                else
                    wgrad_p16_item<2, NW, NITI_WG_D4, true>(g, tile, -1, kg_begin, kg_end, kpw, lds4, quad);
                __syncthreads();  // (the next item may be of the merged form: all four quarters)
                continue;
            }
        }
        switch (ow) {
            case 8: wgrad_p16_item<8, NW, NITI_WG_D8>(g, tile, slab, kg_begin, kg_end, kpw, lds4); break;
            case 16: wgrad_p16_item<16, NW, 8>(g, tile, slab, kg_begin, kg_end, kpw, lds4); break;
            case 4: wgrad_p16_item<4, NW, NITI_WG_D4>(g, tile, slab, kg_begin, kg_end, kpw, lds4); break;
            default: wgrad_p16_item<2, NW, NITI_WG_D4>(g, tile, slab, kg_begin, kg_end, kpw, lds4); break;
        }
        __syncthreads();  // every wave has read its part of the merge buffer and the block-max scratch
    }
}

// NHWC16 [P][CP] -> P16 [P/16][CP][16].  A 16-pixel block is 16 * CP contiguous bytes on both
// sides (16 rows of CP channels in, CP rows of 16 pixels out), so each workgroup copies whole
// blocks into LDS with 16-byte coalesced loads and writes them back transposed: a lane gathers one
// channel's 16 pixels with byte reads (4 lanes share each LDS dword, no bank conflicts) and stores
// one 16-byte chunk, consecutive lanes consecutive chunks.  CP is a power of two from 32 to 1024:
// a workgroup takes 256 / CP blocks (CP <= 256) or one block (CP > 256).  One launch serves up to
// P16_MAX_JOBS tensors, each owning a contiguous range of workgroups.
__global__ void __launch_bounds__(256) nhwc16_to_p16_kernel(P16Jobs J) {
    __shared__ __attribute__((aligned(16))) int8_t tile[16 * 1024];
    p16_convert_block(J, blockIdx.x, tile);
}

// any CP % 16 == 0: one thread per (16-pixel block, 16-channel chunk), a 16 x 16 byte transpose
// in registers
__global__ void nhwc16_to_p16_any_kernel(const int8_t* __restrict__ in, int64_t blocks, int cp,
                                         int8_t* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int cc = cp / 16;
    if (e >= blocks * cc) return;
    const int64_t b = e / cc;
    const int c16 = (int)(e - b * cc);
    v16c px[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) px[p] = *(const v16c*)(in + ((b * 16 + p) * cp + c16 * 16));
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        v16c o;
#pragma unroll
        for (int p = 0; p < 16; ++p) o[p] = px[p][k];
        *(v16c*)(out + (b * cp + c16 * 16 + k) * 16) = o;
    }
}

// the power-of-two-CP jobs as one P16Jobs launch of *wgs workgroups; any other CP runs its own
// generic launch here
hipError_t p16_jobs_build(const P16Conv* jobs, int n, hipStream_t st, P16Jobs* out, uint32_t* wgs_out) {
    if (n < 0 || n > P16_MAX_JOBS) return hipErrorInvalidValue;
    P16Jobs& J = *out;
    J = P16Jobs{};
    uint32_t wg = 0;
    for (int i = 0; i < n; ++i) {
        const P16Conv& c = jobs[i];
        if (c.cp <= 0 || c.cp % 16 != 0 || c.pixels < 0 || c.pixels % 16 != 0) return hipErrorInvalidValue;
        if (c.pixels == 0) continue;
        const int64_t blocks = c.pixels / 16;
        if ((c.cp & (c.cp - 1)) != 0 || c.cp < 32 || c.cp > 1024) {  // not a power of two: generic kernel
            const int64_t t = blocks * (c.cp / 16);
            hipLaunchKernelGGL(nhwc16_to_p16_any_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, st, c.in,
                               blocks, c.cp, c.out);
            continue;
        }
        int lg = 0;
        while ((1 << lg) < c.cp) ++lg;
        const int bpw = lg < 8 ? 1 << (8 - lg) : 1;
        const int64_t wgs = (blocks + bpw - 1) / bpw;
        if ((int64_t)wg + wgs > 0x7fffffff) return hipErrorInvalidValue;
        J.j[J.n++] = P16Job{c.in, c.out, blocks, lg, wg};
        wg += (uint32_t)wgs;
    }
    *wgs_out = wg;
    return hipGetLastError();
}

hipError_t nhwc16_to_p16_many(const P16Conv* jobs, int n, hipStream_t st) {
    P16Jobs J;
    uint32_t wg = 0;
    hipError_t e = p16_jobs_build(jobs, n, st, &J, &wg);
    if (e != hipSuccess) return e;
    if (J.n > 0) hipLaunchKernelGGL(nhwc16_to_p16_kernel, dim3(wg), dim3(256), 0, st, J);
    return hipGetLastError();
}

hipError_t nhwc16_to_p16(const int8_t* in, int64_t pixels, int cp, int8_t* out, hipStream_t st) {
    const P16Conv c{in, pixels, cp, out};
    return nhwc16_to_p16_many(&c, 1, st);
}

// ---- host side --------------------------------------------------------------------------------
static unsigned long long* g_wg_stamps = nullptr;  // diagnostic builds: armed by niti_diag_wgrad_stamps
void wgrad_stamps_arm(unsigned long long* buf) { g_wg_stamps = buf; }

static bool p16_geom(const ConvGeom& g, WgP16* t) {
    if (g.kh != 3 || g.kw != 3 || g.sh != 1 || g.sw != 1 || g.dh != 1 || g.dw != 1) return false;
    if (g.pt != 1 || g.pl != 1 || g.pb != 1 || g.pr != 1) return false;
    if (g.cip % 32 != 0 || g.cop % 32 != 0) return false;
    // a 16-pixel block is whole rows (OW 8 / 16) or whole images (OW 4 / 2)
    const int ow = g.ow, oh = g.oh;
    // square images (the block-in-image masks use a power-of-two block count: 4 for 8x8, 16 for 16x16)
    if (oh != ow || !(ow == 8 || ow == 16 || ow == 4 || ow == 2)) return false;
    const int64_t po = (int64_t)g.n * oh * ow;
    if (po % 32 != 0) return false;  // whole K groups (two blocks)
    if (po * g.cip > 0x7fffffff || po * g.cop > 0x7fffffff) return false;
    WgP16 w{};
    w.CIP = g.cip;
    w.COP = g.cop;
    w.c_out = g.c_out;
    w.ldc = (int64_t)9 * g.cip;
    w.bpi = ow == 8 ? oh / 2 : ow == 16 ? oh : 1;
    w.xbytes = (uint32_t)(po * g.cip);
    w.dybytes = (uint32_t)(po * g.cop);
    w.kg_total = (int)(po / 32);
    w.tiles_ci = g.cip / 32;
    w.tiles = (g.cop / 32) * w.tiles_ci;
    w.fTci = make_fastdiv((uint32_t)w.tiles_ci);
    *t = w;
    return true;
}

bool conv_wgrad_p16_ok(const ConvGeom& g) {
    WgP16 t;
    return p16_geom(g, &t);
}

// default split count: one block per CU, at most 8 partial tiles per combine
int conv_wgrad_p16_splits(const ConvGeom& g) {
    WgP16 t;
    if (!p16_geom(g, &t)) return 0;
    const int kpi = g.ow == 8 ? 2 : g.ow == 16 ? 8 : 1;
    int s = std::max(1, 256 / t.tiles);
    s = std::min(s, 8);
    s = std::min(s, std::max(1, t.kg_total / kpi));
    return s;
}

static int64_t p16_slab_stride(const ConvGeom& g) {
    // an odd number of 4 KiB pages between slabs: the S reads of one element hit different channels
    const int64_t bytes = (int64_t)g.c_out * 9 * g.cip * 4;
    return ((bytes + 4095) / 4096 | 1) * 1024;
}

size_t conv_wgrad_p16_workspace(const ConvGeom& g, int splits) {
    WgP16 t;
    if (!p16_geom(g, &t)) return 0;
    if (splits <= 0) splits = conv_wgrad_p16_splits(g);
    return splits > 1 ? (size_t)splits * p16_slab_stride(g) * 4 : 0;
}

hipError_t conv_wgrad_p16(const ConvGeom& g, const int8_t* x_p16, const int8_t* dy_p16, int32_t* acc,
                          uint32_t* amax, void* ws, size_t ws_bytes, int splits, hipStream_t st, hipEvent_t ev_b,
                          hipEvent_t ev_e, unsigned long long* span, SgdJob* defer) {
    WgP16 t;
    if (!p16_geom(g, &t)) return hipErrorInvalidValue;
    if (splits <= 0) splits = conv_wgrad_p16_splits(g);
    if (splits < 1 || splits > 64) return hipErrorInvalidValue;
    t.x = x_p16;
    t.dy = dy_p16;
    // splits and wave runs cover whole images (K groups per image: 2 for 8x8, 8 for 16x16)
    const int kpi = g.ow == 8 ? 2 : g.ow == 16 ? 8 : 1;
    auto round_kpi = [&](int v) { return (v + kpi - 1) / kpi * kpi; };
    t.kg_per_split = round_kpi((t.kg_total + splits - 1) / splits);
    t.splits = (t.kg_total + t.kg_per_split - 1) / t.kg_per_split;  // no empty split
    t.kg_per_wave = round_kpi((t.kg_per_split + P16_WAVES - 1) / P16_WAVES);
    if (t.splits > 1 && (ws == nullptr || ws_bytes < (size_t)t.splits * p16_slab_stride(g) * 4))
        return hipErrorInvalidValue;
    t.fTiles = make_fastdiv((uint32_t)t.tiles);
    t.C = acc;
    t.amax = amax;
    t.slab = (int32_t*)ws;
    t.slab_stride = p16_slab_stride(g);
    t.span = span;
    t.stamps = g_wg_stamps;
    constexpr int NW = P16_WAVES;
    const dim3 grid((unsigned)(t.tiles * t.splits));
    auto launch = [&](auto k) {
        if (ev_b != nullptr && ev_e != nullptr)
            hipExtLaunchKernelGGL(k, grid, dim3(NW * 64), 0, st, ev_b, ev_e, 0, t);
        else
            hipLaunchKernelGGL(k, grid, dim3(NW * 64), 0, st, t);
    };
    switch (g.ow) {
        case 8: launch(wgrad_p16_kernel<8, NW, NITI_WG_D8>); break;
        case 16: launch(wgrad_p16_kernel<16, NW, 8>); break;
        case 4: launch(wgrad_p16_kernel<4, NW, NITI_WG_D4>); break;
        default: launch(wgrad_p16_kernel<2, NW, NITI_WG_D4>); break;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && t.splits > 1) {
        const int64_t n = (int64_t)g.c_out * 9 * g.cip;
        if (defer != nullptr) {  // the NITI_SGD launch combines the slabs (sgd_update_many)
            defer->slab = t.slab;
            defer->splits = t.splits;
            defer->slab_stride = t.slab_stride;
            defer->slab_n = n;
        } else {
            e = splitk_reduce_linear(t.slab, t.splits, n, t.slab_stride, acc, amax, st);
        }
    }
    return e;
}

// The schedule of wgrad_p16_many_kernel.  A layer's K range is cut into whole-image runs of about
// t K groups (conv_wgrad_p16's rounding; at most what its slab bytes hold), every (tile, run) is an
// item, and the items go longest first into the list with the least work so far.  An item's cost
// is its K groups plus P16_ITEM_FIXED: the prologue, merge and output of an item are about 6.8k
// cycles against 346 per K group.
//
// Quad items (quad_kg > 0): an unsplit layer of 2x2 / 4x4 maps whose whole K range is at most
// quad_kg K groups is cut into items of four consecutive tiles (the last may hold fewer), one tile
// per wave.  Such an item's K time is one wave's -- the layer's kg_total, not four times it -- and
// its fixed phases are the prologue, one wave's LDS write and the four output passes.  Stamps of
// one item per workgroup on a 512 -> 512 layer of 2x2 maps at batch 256 (tools/wg_quad_diag.py,
// cycles): merged form prologue 712, K loop 4438, LDS write and the wait for the slowest wave 1812,
// sum 657, output 2851 -- 6.0k outside the K loop (6.8k inside a step's launch, above: 20 K groups);
// quad form prologue 696, K loop 12640 (32 K groups), LDS write 1900, output 6922 -- 9.6k outside
// the K loop: 28 K groups at 346 cycles.  (Weights of 24 to 48 gave the same launch time, 40.1-40.5
// us per VGG-11 batch-256 step.)
constexpr int P16_ITEM_FIXED = 20;
constexpr int P16_QUAD_FIXED = 28;

hipError_t conv_wgrad_p16_many_build(const WgP16Job* jobs, int n, int blocks, int t, int quad_kg, WgP16Many* out) {
    out->clear();
    if (jobs == nullptr || n < 1 || n > P16_MANY_MAX_JOBS || blocks < 1 || blocks > 4096 || t < 1 || quad_kg < 0)
        return hipErrorInvalidValue;
    if (!P16_QUAD_OK) quad_kg = 0;
    std::vector<WgP16Desc> descs((size_t)n);
    std::vector<WgP16Item> items;
    for (int j = 0; j < n; ++j) {
        const WgP16Job& jb = jobs[j];
        const ConvGeom& g = jb.g;
        WgP16 w;
        if (!p16_geom(g, &w) || !jb.x_p16 || !jb.dy_p16 || !jb.acc) return hipErrorInvalidValue;
        const int kpi = g.ow == 8 ? 2 : g.ow == 16 ? 8 : 1;
        auto round_kpi = [&](int v) { return (v + kpi - 1) / kpi * kpi; };
        const int64_t stride = p16_slab_stride(g);
        const int64_t room = jb.slab != nullptr ? (int64_t)(jb.slab_bytes / ((size_t)stride * 4)) : 0;
        int s = std::max(1, (w.kg_total + t / 2) / t);
        s = std::min(s, std::max(1, w.kg_total / kpi));
        s = (int)std::min<int64_t>(std::min(s, 64), room >= 2 ? room : 1);
        const int kg_per_split = round_kpi((w.kg_total + s - 1) / s);
        s = (w.kg_total + kg_per_split - 1) / kg_per_split;  // no empty split
        w.x = jb.x_p16;
        w.dy = jb.dy_p16;
        w.kg_per_split = kg_per_split;
        w.kg_per_wave = round_kpi((kg_per_split + P16_WAVES - 1) / P16_WAVES);
        w.splits = s;
        w.fTiles = make_fastdiv((uint32_t)w.tiles);
        w.C = jb.acc;
        w.amax = jb.amax;
        w.slab = s > 1 ? jb.slab : nullptr;
        w.slab_stride = stride;
        w.span = nullptr;
        w.stamps = g_wg_stamps;  // (diagnostic builds: the block's last item leaves its marks)
        descs[j] = WgP16Desc{w, g.ow, 0};
        out->splits[j] = s;
        out->slab_stride[j] = stride;
        if (s == 1 && g.ow <= 4 && w.kg_total <= quad_kg) {
            for (int t0 = 0; t0 < w.tiles; t0 += P16_WAVES)
                items.push_back(WgP16Item{j, t0, -1, 0, w.kg_total, w.kg_total, std::min(P16_WAVES, w.tiles - t0), 0});
            continue;
        }
        for (int sp = 0; sp < s; ++sp) {
            const int kb = sp * kg_per_split, ke = std::min(w.kg_total, kb + kg_per_split);
            const int kpw = round_kpi((ke - kb + P16_WAVES - 1) / P16_WAVES);
            for (int tile = 0; tile < w.tiles; ++tile)
                items.push_back(WgP16Item{j, tile, s > 1 ? sp : -1, kb, ke, kpw, 0, 0});
        }
    }
    // longest first (ties: table order, which keeps a layer's tiles together), each into the
    // lightest list so far (ties: the lowest block)
    std::vector<int> order(items.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    auto len = [&](int i) { return items[i].kg_end - items[i].kg_begin; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len(a) > len(b); });
    std::vector<int64_t> load((size_t)blocks, 0);
    std::vector<int> kg((size_t)blocks, 0);
    std::vector<std::vector<int>> lists((size_t)blocks);
    for (int i : order) {
        const int b = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        lists[b].push_back(i);
        load[b] += len(i) + (items[i].quad > 0 ? P16_QUAD_FIXED : P16_ITEM_FIXED);
        kg[b] += len(i);
        out->n_quads += items[i].quad > 0;
    }
    const size_t starts_off = (descs.size() * sizeof(WgP16Desc) + 63) / 64 * 64;
    const size_t items_off = (starts_off + (size_t)(blocks + 1) * sizeof(int) + 63) / 64 * 64;
    const size_t bytes = items_off + items.size() * sizeof(WgP16Item);
    unsigned char* tb = (unsigned char*)calloc(bytes, 1);
    if (tb == nullptr) return hipErrorOutOfMemory;
    memcpy(tb, descs.data(), descs.size() * sizeof(WgP16Desc));
    int* starts = (int*)(tb + starts_off);
    WgP16Item* it = (WgP16Item*)(tb + items_off);
    int k = 0;
    for (int b = 0; b < blocks; ++b) {
        starts[b] = k;
        for (int i : lists[b]) it[k++] = items[i];
    }
    starts[blocks] = k;
    out->table = tb;
    out->table_bytes = bytes;
    out->starts_off = starts_off;
    out->items_off = items_off;
    out->blocks = blocks;
    out->n_jobs = n;
    out->n_items = k;
    out->max_list_kg = *std::max_element(kg.begin(), kg.end());
    return hipSuccess;
}

// the schedule as plain integers, for host-side checks: per item {job, first tile, tiles (0: the
// merged form, one tile), slab, kg_begin, kg_end, kg_per_wave, form (1: quad)}
int conv_wgrad_p16_many_items(const WgP16Many& m, int* items8, int cap_items, int* starts, int cap_starts) {
    if (m.table == nullptr || cap_items < m.n_items || cap_starts < m.blocks + 1) return -1;
    const WgP16Item* it = (const WgP16Item*)(m.table + m.items_off);
    for (int i = 0; i < m.n_items; ++i) {
        const int row[8] = {it[i].job,      it[i].tile,   it[i].quad,        it[i].slab,
                            it[i].kg_begin, it[i].kg_end, it[i].kg_per_wave, it[i].quad > 0};
        memcpy(items8 + 8 * i, row, sizeof row);
    }
    memcpy(starts, m.table + m.starts_off, (size_t)(m.blocks + 1) * sizeof(int));
    return m.n_items;
}

static std::atomic<unsigned long long> g_many_launches{0};
unsigned long long conv_wgrad_p16_many_launches() { return g_many_launches.load(); }

hipError_t conv_wgrad_p16_many(const WgP16Many& m, const void* table_dev, hipStream_t st) {
    if (m.table == nullptr || table_dev == nullptr || m.blocks < 1) return hipErrorInvalidValue;
    ++g_many_launches;
    const unsigned char* base = (const unsigned char*)table_dev;
    hipLaunchKernelGGL(wgrad_p16_many_kernel<P16_WAVES>, dim3((unsigned)m.blocks), dim3(P16_WAVES * 64), 0, st,
                       (const WgP16Desc*)base, (const int*)(base + m.starts_off),
                       (const WgP16Item*)(base + m.items_off));
    return hipGetLastError();
}

}  // namespace niti
