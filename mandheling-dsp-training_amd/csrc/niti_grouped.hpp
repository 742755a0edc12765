// niti_grouped.hpp -- what the grouped conv kernel families share (niti_grouped.hip: group widths 16, 32, 64 on the
// 16x16x64 MFMA; niti_grouped_narrow.hip: 4 and 8 on the 4x4x4 block MFMA; niti_grouped_packed.hip: the other
// multiples of 8 up to 128, K packed across taps): the launch arguments, the 4 x 4 byte transpose, pass 1's
// requantisation of a lane's four accumulators and pass 0's range.  And, for the host: the width rule (gc_width:
// which family takes a group width, and how it lays out its weights and maps) and the record each family exports
// for the one host front (niti_grouped_host.hip).
#pragma once
#include "niti_device.hpp"
#include "niti_sgd.hpp"

namespace niti {

// ---- the width rule: the one place that says which group width cg belongs to which family --------------------
enum GcFamily { GC_NONE, GC_WIDE, GC_NARROW, GC_PACKED };
struct GcWidth {
    GcFamily family;  // GC_NONE: no kernel takes the width
    int cgp;          // the weight pitch: w, its int32 gradient and the slabs are [c_out][9][cgp]
    bool pitch16;     // the maps' channel pitch: cip == cop == C rounded up to 16 (else C itself)
    bool c16;         // a chain network's layer of this width needs c_in % 16 == 0
    int rule;         // the lowest CHAIN_RULE_* whose entry points admit the width
};
inline GcWidth gc_width(int cg) {
    if (cg == 16 || cg == 32 || cg == 64) return {GC_WIDE, cg, false, false, CHAIN_RULE_WIDE};
    if (cg == 4 || cg == 8) return {GC_NARROW, 16, false, true, CHAIN_RULE_NARROW};
    if (cg % 8 == 0 && cg >= 24 && cg <= 128) return {GC_PACKED, cg, true, false, CHAIN_RULE_PACKED};
    return {GC_NONE, cg, false, false, 0};
}

struct GcActArgs;
struct GcWgArgs;
using GcActKern = void (*)(GcActArgs);
using GcWgKern = void (*)(GcWgArgs);
// What a kernel family tells the host front: its tiling, its grid and its kernels.  A workgroup takes 4 output
// rows (a band) of one column segment everywhere.
struct GcKernels {
    int (*segs)(int cols, int cg, int stride);  // the column segments of `cols` unit pixels
    unsigned (*grid_y)(int C, int groups);      // gridDim.y of every launch
    unsigned (*wgrad_z)(int cg);                // gridDim.z of the weight gradient
    int min_workgroups;  // the weight gradient's slab cap is at least min_workgroups / grid_y (0: no such term)
    GcActKern (*act)(int cg, int stride, bool dgrad, int pass);
    GcWgKern (*wgrad)(int cg, int stride);
};
// niti_grouped.hip, _narrow.hip, _packed.hip (behind a host function: a constant at namespace scope would be
// emitted into the device code as well)
const GcKernels& gc_wide();
const GcKernels& gc_narrow();
const GcKernels& gc_packed();

constexpr int GC_MAX_SLABS = 1024;
constexpr size_t GC_SLAB_BYTES = size_t(4) << 20;  // of all slabs, past 64 of them: the combine reads every one

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

struct GcActArgs {
    const int8_t* x;  // [n][ih][iw][C]
    const int8_t* w;  // [C][9][cg] (group widths 4, 8: [C][9][16])
    int8_t* out;      // [n][oh][ow][C]
    const int8_t* relu_mask;
    uint32_t xbytes, wbytes;
    int ih, iw, oh, ow, C, pad, relu;
    int bands, segs;  // row bands and column segments of an image
    uint32_t* amax;
    const int8_t* exp_in;
    const int8_t* wscale;
    int8_t* exp_out;
    int cp;  // niti_grouped_packed.hip: the channel pitch of x, out and relu_mask (C rounded up to 16)
};

struct GcWgArgs {
    const int8_t* x;   // [n][h][w][C]
    const int8_t* dy;  // [n][oh][ow][C]
    int32_t* slab;     // [gridDim.x][C][9][cg] (group widths 4, 8: [C][9][16])
    uint32_t xbytes, dbytes;
    int h, w, oh, ow, C, pad;
    int bands, segs;  // row bands and column segments of an image
    int units;        // n * bands * segs
    int cp;           // niti_grouped_packed.hip: the channel pitch of x and dy (C rounded up to 16)
};

// pass 1's shift from the published range (NITI_Conv_Int8.cpp:260-307), the exponent written by one thread
struct Gc2Quant {
    int s;
    bool raw;
};
template <int PASS>
__device__ __forceinline__ Gc2Quant gc2_quant(const GcActArgs& a, uint32_t gm) {
    Gc2Quant z{2, true};
    if (PASS == 1) {
        const int shift = __builtin_amdgcn_readfirstlane(bitwidth_of(wave_max(gm))) - 7;
        z.s = shift > 1 ? shift : 2;
        z.raw = shift <= 0;
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && a.exp_out != nullptr) {
            const int inc = shift > 1 ? shift : (shift == 1 ? 2 : 0);
            *a.exp_out = (int8_t)((a.exp_in ? (int)*a.exp_in : 0) + (a.wscale ? (int)*a.wscale : 0) + inc);
        }
    }
    return z;
}

// a lane's four accumulators, 4 consecutive channels of one pixel: pass 0 the range, pass 1 one dword of out
template <int PASS>
__device__ __forceinline__ void gc2_emit(const GcActArgs& a, const v4i& acc, size_t off, Gc2Quant z, uint32_t& m) {
    if (PASS == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) m = max(m, uabs32(acc[e]));
    } else {
        uint32_t mk = 0;
        if (a.relu_mask != nullptr) mk = *(const uint32_t*)(a.relu_mask + off);
        uint32_t o = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int32_t v = z.raw ? (int32_t)(int8_t)acc[e] : psto_fast(acc[e], z.s);
            if (a.relu && v < 0) v = 0;
            if (a.relu_mask != nullptr && (int8_t)(mk >> (8 * e)) <= 0) v = 0;
            o |= ((uint32_t)v & 0xffu) << (8 * e);
        }
        *(uint32_t*)(a.out + off) = o;
    }
}

template <int PASS>
__device__ __forceinline__ void gc2_publish(const GcActArgs& a, uint32_t m, uint32_t* red) {
    if (PASS == 0) {
        m = wave_max(m);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) publish_max(a.amax, max(max(red[0], red[1]), max(red[2], red[3])));
    }
}

}  // namespace niti
