// niti_sgd.hip -- the step's NITI_SGD launches, the .hip counterpart to niti_sgd.hpp (which holds the tile's device
// code, shared with the fused row kernels): sgd_combine_kernel sums the deferred split-K slabs of every layer's weight
// gradient and publishes each range (NITI_RangeEstimate), sgd_update_kernel applies every layer's update in one launch
// (g = gradient rule(acc), w <- clip(w - g) in OHWI16 and transposed in IHWO16), and update_bits_set_kernel writes the
// per-layer update-bits words (include/niti_hip.h).  Entry points: sgd_combine_many, sgd_update_many, sgd_update,
// update_bits_set (niti_kernels.hpp).
#include "niti_device.hpp"
#include "niti_kernels.hpp"
#include "niti_sgd.hpp"

namespace niti {

// Fused NITI_SGD step on a 64(co) x 64(ci) tile of one tap: g = gradient rule(acc), w <- clip(w - g)
// in OHWI16, and the updated weights also written transposed (IHWO16, the input-gradient B
// operand) through an LDS tile -- the transposed copy never needs a pass of its own.
// One 64 (co) x 64 (ci) tile of one tap: g = rule(acc, range), w <- clip(w - g, +-127) in OHWI16,
// the same tile transposed through LDS into IHWO16 (the input-gradient operand), g to g_out.
// bw: NITI_RangeEstimate of the job's gradient (read once per job by the caller)
// (sgd_tile: niti_sgd.hpp)

// Every layer's NITI_SGD update of a step in one launch: block b belongs to the job whose
// [start, start + tiles) range holds it (the updates are independent; the input gradients
// that read the old weights have all run by then).
// The deferred split-K combines of a step's P16 weight gradients, all layers in one launch ahead
// of the update (one launch instead of one reduce per layer, each of which left the chip mostly
// idle: 576 blocks of a few loads each): chunk c (1024 elements of one job's acc, 4 per thread) =
// the sum of the job's slabs, its max into the job's range.  A small gradient over many splits
// takes splitk_reduce's form instead: G lanes per 16-byte group, each summing every G-th split,
// a shuffle tree to finish (a chunk is then 1024 / G elements; sgd_combine_lanes).
// (A grid barrier inside the update
// launch instead measured +275 us per VGG-11 step: 1536-2048 arrivals on one counter.)
__global__ void __launch_bounds__(256) sgd_combine_kernel(SgdJobs jobs) {
    const int chunks = jobs.cstart[jobs.n];
    // a block's chunks ascend, so its jobs do too: the running max of the current job is
    // published once when the block leaves it (one atomic per wave per job, not per chunk --
    // ResNet-18's ~15 K chunks of per-chunk atomics on a few range words cost ~50 us)
    uint32_t m = 0;
    int cur = -1;
    for (int c = blockIdx.x; c < chunks; c += gridDim.x) {
        int j = 0;
        while (j + 1 < jobs.n && c >= jobs.cstart[j + 1]) ++j;
        if (j != cur) {
            if (cur >= 0) {
                const uint32_t w = wave_max(m);
                if ((threadIdx.x & 63) == 0) publish_max(const_cast<uint32_t*>(jobs.job[cur].amax), w);
            }
            cur = j;
            m = 0;
        }
        const SgdJob& J = jobs.job[j];
        // G lanes share an element group and split its slabs among them (sgd_combine_lanes: 1 for
        // a job with a few chunks per split; block-uniform, so every lane reaches the shuffles)
        const int G = sgd_combine_lanes(J.splits, J.slab_n);
        const int g = threadIdx.x & (G - 1);
        const int64_t e = ((int64_t)(c - jobs.cstart[j]) * (256 / G) + threadIdx.x / G) * 4;
        int64_t de = e;  // the acc element this slab element sums into
        bool live = J.slab != nullptr && e < J.slab_n;
        if (live && J.slab_map == 1) {  // SlabTapsBlocked (splitk_reduce's map), on 16-byte units
            const uint32_t u = (uint32_t)(e >> 2);
            const uint32_t tile = u / 4608u, rem = u - tile * 4608u;
            const uint32_t row = rem / 72u, rc = rem - row * 72u;
            const uint32_t t = rc / 8u, part = rc - t * 8u;
            FastDiv ft;
            ft.m = J.tb_m;
            ft.s = J.tb_s;
            const uint32_t tco = fdiv(ft, tile), tci = tile - tco * (uint32_t)J.tb_tiles_ci;
            const int co = (int)(tco * 64u + row);
            live = co < J.co;
            de = ((int64_t)co * J.tb_ld4 + t * J.tb_cip4 + tci * 8u + part) * 4;
        }
        v4i s = {0, 0, 0, 0};
        if (live) {
            const v4i* base = (const v4i*)(J.slab + e);
            const int64_t st4 = J.slab_stride / 4;
            for (int z0 = g; z0 < J.splits; z0 += 8 * G) {  // up to 8 independent loads in flight
                v4i v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int z = z0 + q * G;
                    v[q] = z < J.splits ? __builtin_nontemporal_load(base + (int64_t)z * st4) : v4i{0, 0, 0, 0};
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) s += v[q];
            }
        }
        for (int o = G >> 1; o > 0; o >>= 1) {  // (the lanes of a group are live together)
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] += __shfl_xor(s[q], o, 64);
        }
        if (live && g == 0) {
            *(v4i*)(const_cast<int32_t*>(J.acc) + de) = s;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t u = uabs32(s[q]);
                m = m > u ? m : u;
            }
        }
    }
    if (cur >= 0) {
        const uint32_t w = wave_max(m);
        if ((threadIdx.x & 63) == 0) publish_max(const_cast<uint32_t*>(jobs.job[cur].amax), w);
    }
}

// bits: the update-bits table the jobs with rule < 0 name a word of (sgd_rule_word; a launch without
// one passes any readable word: word 0 is loaded, and ignored, for a job with an immediate rule)
__global__ void sgd_update_kernel(SgdJobs jobs, int total, const int32_t* __restrict__ bits) {
    __shared__ int8_t T[64][64 + 4];
    // a block takes tiles b, b + gridDim, ...: one resident wave of blocks instead of a full
    // wave plus a straggling partial one.  The next tile's operands are loaded before this one is
    // finished, and a tile's loads are issued before its job's range is read (the range word's
    // dependent read and wave reduction then overlap the operand fetch).
    struct Tile {
        int j, ci0, co0, k;
    };
    auto locate = [&](int bb) {
        Tile t;
        int b = bb, j = 0;
        while (j + 1 < jobs.n && b >= jobs.start[j + 1]) ++j;
        const SgdJob& J = jobs.job[j];
        b -= jobs.start[j];
        const int tx = (J.cip + 63) / 64, ty = (J.cop + 63) / 64;
        const int k = b / (tx * ty), rem = b - k * tx * ty;
        t.j = j;
        t.ci0 = (rem % tx) * 64;
        t.co0 = (rem / tx) * 64;
        t.k = k;
        return t;
    };
    int bb = blockIdx.x;
    if (bb >= total) return;
    if (!NITI_SGD_PREFETCH) {  // one tile at a time
        int last_j = -1, bw = 0, rule = 0;
        for (; bb < total; bb += gridDim.x) {
            const Tile t = locate(bb);
            if (t.j != last_j) {
                const int word = sgd_rule_word(jobs.job[t.j], bits);
                bw = bitwidth_of(read_max(jobs.job[t.j].amax));
                rule = sgd_rule_of(jobs.job[t.j], word);
                last_j = t.j;
            }
            if (bb != (int)blockIdx.x) __syncthreads();  // the previous tile's transposed reads are done
            sgd_tile(jobs.job[t.j], bw, rule, t.ci0, t.co0, t.k, T);
        }
        return;
    }
    Tile cur = locate(bb);
    SgdTileIn cin, nin;  // (named, not an indexed pair: a dynamically indexed array would live in scratch)
    sgd_tile_load(jobs.job[cur.j], cur.ci0, cur.co0, cur.k, cin);
    int last_j = -1, bw = 0, rule = 0;
    for (; bb < total; bb += gridDim.x) {
        const int nb = bb + gridDim.x;
        Tile nxt = cur;
        if (nb < total) {
            nxt = locate(nb);
            sgd_tile_load(jobs.job[nxt.j], nxt.ci0, nxt.co0, nxt.k, nin);
        }
        if (cur.j != last_j) {
            const int word = sgd_rule_word(jobs.job[cur.j], bits);
            bw = bitwidth_of(read_max(jobs.job[cur.j].amax));
            rule = sgd_rule_of(jobs.job[cur.j], word);
            last_j = cur.j;
        }
        if (bb != (int)blockIdx.x) __syncthreads();  // the previous tile's transposed reads are done
        sgd_tile_finish(jobs.job[cur.j], bw, rule, cur.ci0, cur.co0, cur.k, cin, T);
        cur = nxt;
        cin = nin;
    }
}

// the deferred combines of sgd_update_many alone (the autotuner times a weight-gradient set with them)
hipError_t sgd_combine_many(const SgdJob* jobs, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (n > SGD_MAX_JOBS) return hipErrorInvalidValue;
    SgdJobs J{};
    J.n = n;
    int chunks = 0;
    for (int i = 0; i < n; ++i) {
        J.job[i] = jobs[i];
        J.cstart[i] = chunks;
        if (jobs[i].slab != nullptr) {
            if (jobs[i].splits < 1 || jobs[i].slab_stride % 4 != 0 || jobs[i].slab_n % 4 != 0) return hipErrorInvalidValue;
            chunks += sgd_combine_chunks(jobs[i].splits, jobs[i].slab_n);
        }
    }
    J.cstart[n] = chunks;
    if (chunks > 0) hipLaunchKernelGGL(sgd_combine_kernel, dim3(chunks < 2048 ? chunks : 2048), dim3(256), 0, st, J);
    return hipGetLastError();
}

hipError_t sgd_update_many(const SgdJob* jobs, int n, hipStream_t st, const int32_t* bits) {
    if (n <= 0) return hipSuccess;
    if (n > SGD_MAX_JOBS) return hipErrorInvalidValue;
    for (int i = 0; i < n; ++i)  // a job that names a table word needs the table
        if (jobs[i].rule < 1 && bits == nullptr) return hipErrorInvalidValue;
    SgdJobs J{};
    J.n = n;
    int total = 0, chunks = 0;
    for (int i = 0; i < n; ++i) {
        J.job[i] = jobs[i];
        J.start[i] = total;
        J.cstart[i] = chunks;
        total += ((jobs[i].cip + 63) / 64) * ((jobs[i].cop + 63) / 64) * jobs[i].kk;
        if (jobs[i].slab != nullptr) {
            if (jobs[i].splits < 1 || jobs[i].slab_stride % 4 != 0 || jobs[i].slab_n % 4 != 0) return hipErrorInvalidValue;
            chunks += sgd_combine_chunks(jobs[i].splits, jobs[i].slab_n);
        }
    }
    J.cstart[n] = chunks;
    if (chunks > 0) {  // the deferred combines first (same stream: the update reads their sums)
        const int cgrid = chunks < 2048 ? chunks : 2048;
        hipLaunchKernelGGL(sgd_combine_kernel, dim3(cgrid), dim3(256), 0, st, J);
    }
    const int grid = total < 1536 ? total : 1536;  // 6 blocks per CU
    // (no table: the first job's range word stands in as the readable word no job uses)
    const int32_t* table = bits != nullptr ? bits : (const int32_t*)jobs[0].amax;
    if (table == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sgd_update_kernel, dim3(grid), dim3(256), 0, st, J, total, table);
    return hipGetLastError();
}

hipError_t sgd_update(const int32_t* acc, const uint32_t* amax, int rule, int co, int ci, int kk, int cip, int cop,
                      int8_t* w, int8_t* wT, int8_t* g_out, hipStream_t st) {
    SgdJob j{acc, amax, rule, co, ci, kk, cip, cop, w, wT, g_out};
    return sgd_update_many(&j, 1, st);
}

// The update-bits words (include/niti_hip.h): word first + t <- v[t], the values travelling as kernel
// arguments so the change is an ordinary launch on the caller's stream (ordered between steps, and
// ahead of a replayed graph's update launches, which read the words); one thread per word.
__global__ void update_bits_set_kernel(int32_t* __restrict__ bits, int first, int count, UpdateBitsArgs v) {
    const int t = (int)threadIdx.x;
    if (t < count) bits[first + t] = v.b[t];
}
hipError_t update_bits_set(int32_t* bits, int first, int count, const int32_t* values, hipStream_t st) {
    if (bits == nullptr || values == nullptr || first < 0 || count < 0) return hipErrorInvalidValue;
    for (int lo = 0; lo < count; lo += UPDATE_BITS_PER_LAUNCH) {
        UpdateBitsArgs v{};
        const int c = count - lo < UPDATE_BITS_PER_LAUNCH ? count - lo : UPDATE_BITS_PER_LAUNCH;
        for (int t = 0; t < c; ++t) v.b[t] = values[lo + t];
        hipLaunchKernelGGL(update_bits_set_kernel, dim3(1), dim3(UPDATE_BITS_PER_LAUNCH), 0, st, bits, first + lo, c, v);
    }
    return hipGetLastError();
}

}  // namespace niti
