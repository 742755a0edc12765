// niti_gridbar.hpp -- the in-kernel grid barrier with the range folded in, shared by the fused row
// kernels (niti_rowconv.hip), the fused residual launch (niti_resnet.hip) and the strategy-4 GEMM
// epilogue (niti_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "niti_kernels.hpp"

#ifndef NITI_BAR_COUNTERS
#define NITI_BAR_COUNTERS 0  // diagnostics: 1 builds the earlier shard-counter form (A/B in one tree)
#endif

namespace niti {

// ---- grid barrier with the range folded in (mode FUSED) ---------------------------------------
// The requantisation needs only the tensor's bit width bw = ceil(log2 max|y|) (NITI_RangeEstimate),
// and the bit width of a max is the max of the bit widths.
//
// Slot form.  Every workgroup owns one 8-byte slot of the state.  Arriving is ONE agent-scope
// relaxed store of (epoch << 32 | bw) into its slot: no read-modify-write, nothing serialised
// against the other arrivals.  One wave per workgroup polls: lane l loads slots l, 64 + l, ... (up
// to four 8-byte loads in flight, 256 slots, per round; a second round for grids past 256), s_sleep
// between polls, bounded.  A poll succeeds when every slot below the grid's size carries this
// launch's epoch; the grid's bw is the max of the slots' low words.
// Tag rule: the tag is the launch's full 32-bit epoch, and a state sees each epoch once (1, 2, 3, ...,
// one per launch; the launchers refuse epoch 0, which is what zeroed state holds).  A slot left by
// any earlier launch therefore never compares equal, whatever grid sizes came before: no parity
// sets, no reset, no truncated tag to wrap.  A driver's own count reaches 0 after 2^32 launches on
// one state: that launch is refused (hipErrorInvalidValue from rowconv_fwd / rowconv_fc /
// residual_fused / act_fused alike, so that one step fails) and the count goes on at 1.  An epoch
// value then comes a second time, 2^32 launches after the first; it could meet its own old slot only
// in a slot no launch in between wrote, i.e. if the state's grid then grew past every grid of those
// 2^32 launches.  The drivers' grids per state repeat step by step, so it cannot; a caller that
// sets epochs itself keeps them distinct per state.
// Capacity: BAR_SLOTS = 512 workgroups, checked on the host where the fused form is admitted
// (grid_bar_fits); on the device a workgroup past it stores nothing and a slot past it is never
// loaded, so such a launch would end in the spin limit, not in an access outside the state.
// Layout (words): slots 0..255 in [0, 512) = lines 0..15, the row kernels' two hint lines at 16 and
// 17 (rowconv_spec_slot), slots 256..511 in [576, 1088) = lines 18..33.
constexpr int BAR_LINE = 32;                   // words per 128-byte line
constexpr int BAR_SLOTS = 512;                 // workgroups a state can hold
constexpr int BAR_HALF = 256;                  // slots per region (one poll round)
constexpr int BAR_HALF_STRIDE = 18 * BAR_LINE;  // words from region 0 to region 1 (past the hint lines)
static_assert(BAR_HALF_STRIDE + BAR_HALF * 2 <= ROWCONV_BAR_WORDS, "barrier state size");
constexpr uint32_t BAR_SPIN_LIMIT = 1u << 22;  // ~seconds of polling: only a non-resident grid reaches it

// host: a grid the barrier state can hold
inline bool grid_bar_fits(int64_t wgs) { return NITI_BAR_COUNTERS != 0 || wgs <= BAR_SLOTS; }

#if !NITI_BAR_COUNTERS

__device__ __forceinline__ unsigned long long* bar_slot(uint32_t* state, int i) {
    return (unsigned long long*)(state + (i >> 8) * BAR_HALF_STRIDE) + (i & (BAR_HALF - 1));
}

// Called by one whole wave of each workgroup (lane 0's bw): the arrival, then -- after whatever
// work the workgroup can do meanwhile -- the wait, which returns the grid's bw to every lane.
__device__ inline void grid_bw_arrive(uint32_t* state, uint32_t epoch, int bw, int lane) {
    const int b = blockIdx.x;
    if (lane == 0 && b < BAR_SLOTS)
        __hip_atomic_store(bar_slot(state, b), ((unsigned long long)epoch << 32) | (uint32_t)bw, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// A workgroup that is not resident never arrives: after spin_limit polls the waiters set *err
// (the Executions return NITI_NO_EXECUTION, the model step reports it: niti_model_rowconv_error)
// and go on with bw = 31 instead of hanging the GPU.  extra (diagnostics): that many more slots
// past the grid's are required to carry the epoch, which nobody writes.
__device__ inline int grid_bw_wait(uint32_t* state, uint32_t epoch, uint32_t* err, uint32_t spin_limit, uint32_t extra,
                            int lane) {
    // slots that must carry this launch's epoch; anything past the capacity can never complete, so
    // BAR_SLOTS + 1 stands for all of it (no 32-bit wrap of grid + extra, at most three rounds a poll)
    const unsigned long long want = (unsigned long long)gridDim.x + extra;
    const uint32_t need = want > (unsigned long long)BAR_SLOTS ? (uint32_t)BAR_SLOTS + 1u : (uint32_t)want;
    const unsigned long long done = (unsigned long long)epoch << 32;
    uint32_t spins = 0, bw = 0;
    for (;;) {
        bool ok = true;
        bw = 0;
        for (uint32_t base = 0; base < need; base += BAR_HALF) {  // wave-uniform
            unsigned long long v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t i = base + j * 64 + lane;
                // beyond need: counts as done; beyond the capacity: never done, never loaded
                v[j] = i >= need ? done
                       : i < (uint32_t)BAR_SLOTS
                           ? __hip_atomic_load(bar_slot(state, (int)i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                           : 0ull;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ok = ok && (uint32_t)(v[j] >> 32) == epoch;
                bw = max(bw, (uint32_t)v[j]);
            }
        }
        if (__all(ok)) break;
        if (++spins > spin_limit) {  // never hang the GPU: flag it and go on (results invalid)
            if (lane == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return 31;
        }
        __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) bw = max(bw, (uint32_t)__shfl_xor((int)bw, o, 64));
    return (int)bw;
}

#else  // NITI_BAR_COUNTERS: the shard-counter form

// Each workgroup ORs (1 << its bw) into its shard word and then adds (1 << 32) to the same 64-bit
// word -- two no-return atomics on ONE address, so they are performed in order and no wait sits
// between them: once a shard's count is complete, every OR of that shard is in.  One wave per
// workgroup polls the 8 shard words (lane s reads shard s) until every count is complete; the global
// bw is the highest bit of the ORed words.  Parity: launch e uses word set e & 1 and zeroes the other
// set for launch e + 1 (the launch that used it last has completed: same stream).
constexpr int BAR_WORDS = 19 * BAR_LINE;  // one parity (8 shard lines used)
static_assert(2 * BAR_WORDS == ROWCONV_BAR_WORDS, "barrier state size");

__device__ __forceinline__ unsigned long long* bar_shard(uint32_t* base, int s) {
    return (unsigned long long*)(base + s * BAR_LINE);
}

__device__ inline void grid_bw_arrive(uint32_t* state, uint32_t epoch, int bw, int lane) {
    uint32_t* S = state + (epoch & 1) * BAR_WORDS;
    const int nwg = gridDim.x, b = blockIdx.x;
    const int nsh = nwg < 8 ? nwg : 8;
    if (b == 0 && lane < 8)  // reset the other parity for the next launch
        __hip_atomic_store(bar_shard(state + ((epoch + 1) & 1) * BAR_WORDS, lane), 0ull, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0) {
        unsigned long long* w = bar_shard(S, b % nsh);
        __hip_atomic_fetch_or(w, 1ull << bw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(w, 1ull << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ inline int grid_bw_wait(uint32_t* state, uint32_t epoch, uint32_t* err, uint32_t spin_limit, uint32_t extra,
                            int lane) {
    uint32_t* S = state + (epoch & 1) * BAR_WORDS;
    const int nwg = gridDim.x;
    const int nsh = nwg < 8 ? nwg : 8;
    // lane s < nsh polls shard s until its count is complete
    const uint32_t expect = lane < nsh ? (uint32_t)((nwg - lane + nsh - 1) / nsh) + (lane == 0 ? extra : 0u) : 0u;
    uint32_t spins = 0;
    unsigned long long v = 0;
    for (;;) {
        v = lane < nsh ? __hip_atomic_load(bar_shard(S, lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        const bool done = (uint32_t)(v >> 32) >= expect;
        if (__all(done)) break;
        if (++spins > spin_limit) {  // never hang the GPU: flag it and go on (results invalid)
            if (lane == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return 31;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    uint32_t bits = (uint32_t)v;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) bits |= __shfl_xor(bits, o, 64);
    return bits == 0u ? 0 : 31 - __clz((int)bits);
}

#endif  // NITI_BAR_COUNTERS

}  // namespace niti
