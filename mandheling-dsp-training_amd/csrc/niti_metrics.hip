// niti_metrics.hip -- head metrics of an evaluation pass: per-image argmax, rank of the label and
// cross-entropy loss from the int8 logits, accumulated into running totals on the device.
//
// The reference's training program prints NITI_LOSS_Int8's value every step
// (tools/train/source/demo/MnistUtils.cpp:100,130; source/backend/cpu/NITI_CPULoss_Int8.cpp:89-125)
// and counts _ArgMax(logits) == label over the test set (MnistUtils.cpp:150-181;
// source/backend/cpu/CPUArgMax.cpp:125-130, a strict > scan: the first maximum wins).
//
// Per image i with 0 <= labels[i] < classes (any other label excludes the image from every total;
// -1 is how a caller pads the last partial batch of a test set):
//   pred[i]  first index of the row maximum over j < classes (written for excluded images too)
//   rank_i   #{j < classes : l[j] > l[label] or (l[j] == l[label] and j < label)}: top-1 correct
//            <=> rank_i == 0 <=> pred[i] == label, top-k correct <=> rank_i < topk
//   loss_i   log(sum_j exp(z_j - z_max)) - (z_label - z_max), z = l * 2^ascale, in double: the
//            differences l[j] - l_max are exact integers, the scaling an exact ldexp.  The reference
//            evaluates the same quantity in float32 through MNNSoftmax's approximate exp; that
//            approximation is not reproduced (the loss is a reported number and feeds nothing back).
//
// Two launches.  head_metrics_rows: one wave64 per image row, each lane up to two 16-byte chunks
// of the row (classes <= 2048) held in registers for the three passes; rows are bounded by
// `classes`, never by `ld`, so whatever the padding lanes hold is never looked at.  The first
// maximum is the wave max of the packed key ((l + 128) << 16) | (0xFFFF - j).  head_metrics_totals:
// one block sums the per-image losses and flags in a fixed order (thread t takes images t, t + 256,
// ...; then a fixed LDS tree) and adds them to the caller's totals with plain loads and stores, in
// stream order: no atomics, so loss_sum is bit-identical from run to run.
#include "niti_kernels.hpp"

namespace niti {

namespace {

constexpr int HM_ROWS = 4;  // image rows (waves) per 256-thread block
constexpr int HM_MAXC = 2048;
constexpr int HM_CHUNKS = HM_MAXC / 16 / 64;  // 16-byte chunks per lane

template <class T>
__device__ inline T wave_xor(T v, int o) {
    return __shfl_xor(v, o, 64);
}

// VEC: rows are 16-byte aligned (ld % 16 == 0 and an aligned base), one 16-byte load per chunk --
// the chunk lies inside the row's ld bytes; else byte loads of the lanes below `classes` only
template <bool VEC>
__global__ void __launch_bounds__(256) head_metrics_rows_kernel(const int8_t* __restrict__ logits, int batch,
                                                                int classes, int ld,
                                                                const int8_t* __restrict__ ascale_p,
                                                                const int32_t* __restrict__ labels, int topk,
                                                                int32_t* __restrict__ pred,
                                                                double* __restrict__ loss_user,
                                                                double* __restrict__ loss_ws,
                                                                int32_t* __restrict__ flag_ws) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * HM_ROWS + (threadIdx.x >> 6);
    if (i >= batch) return;  // (whole waves; no block barrier below)
    const int as = (int)*ascale_p;
    const int label = labels[i];
    const bool counted = label >= 0 && label < classes;
    const int8_t* L = logits + (int64_t)i * ld;
    const int lv = counted ? (int)L[label] : 0;
    int v[HM_CHUNKS][16];
#pragma unroll
    for (int c = 0; c < HM_CHUNKS; ++c) {
        const int j0 = (lane + 64 * c) * 16;
        if (j0 < classes) {
            if (VEC) {
                const int4 q = *reinterpret_cast<const int4*>(L + j0);
                const uint32_t w[4] = {(uint32_t)q.x, (uint32_t)q.y, (uint32_t)q.z, (uint32_t)q.w};
#pragma unroll
                for (int e = 0; e < 16; ++e) v[c][e] = (int)(int8_t)(w[e >> 2] >> (8 * (e & 3)));
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) v[c][e] = j0 + e < classes ? (int)L[j0 + e] : -128;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) v[c][e] = -128;
        }
    }
    // first maximum and the label's rank (all integer)
    uint32_t key = 0;
    int rank = 0;
#pragma unroll
    for (int c = 0; c < HM_CHUNKS; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int j = (lane + 64 * c) * 16 + e;
            if (j < classes) {
                const uint32_t k = ((uint32_t)(v[c][e] + 128) << 16) | (uint32_t)(0xFFFF - j);
                key = k > key ? k : key;
                rank += (v[c][e] > lv || (v[c][e] == lv && j < label)) ? 1 : 0;
            }
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t k = wave_xor(key, o);
        key = k > key ? k : key;
        rank += wave_xor(rank, o);
    }
    const int mx = (int)(key >> 16) - 128;
    const int first = 0xFFFF - (int)(key & 0xFFFF);
    // sum_j exp((l_j - l_max) * 2^ascale): per lane in index order, then a fixed butterfly
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < HM_CHUNKS; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int j = (lane + 64 * c) * 16 + e;
            if (j < classes) s += exp(ldexp((double)(v[c][e] - mx), as));
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += wave_xor(s, o);
    if (lane == 0) {
        const double loss = counted ? log(s) - ldexp((double)(lv - mx), as) : 0.0;
        if (pred != nullptr) pred[i] = first;
        if (loss_user != nullptr) loss_user[i] = loss;
        loss_ws[i] = loss;
        flag_ws[i] = counted ? 1 | (rank == 0 ? 2 : 0) | (rank < topk ? 4 : 0) : 0;
    }
}

__global__ void __launch_bounds__(256) head_metrics_totals_kernel(const double* __restrict__ loss,
                                                                  const int32_t* __restrict__ flags, int batch,
                                                                  niti_eval_totals* __restrict__ totals) {
    __shared__ double sl[256];
    __shared__ unsigned long long sc[3][256];
    const int tid = threadIdx.x;
    double l = 0.0;
    unsigned long long n = 0, t1 = 0, tk = 0;
    for (int i = tid; i < batch; i += 256) {
        const int f = flags[i];
        l += loss[i];  // (0 for an excluded image)
        n += f & 1;
        t1 += (f >> 1) & 1;
        tk += (f >> 2) & 1;
    }
    sl[tid] = l;
    sc[0][tid] = n;
    sc[1][tid] = t1;
    sc[2][tid] = tk;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            sl[tid] += sl[tid + o];
            sc[0][tid] += sc[0][tid + o];
            sc[1][tid] += sc[1][tid + o];
            sc[2][tid] += sc[2][tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        totals->images += sc[0][0];
        totals->top1 += sc[1][0];
        totals->topk += sc[2][0];
        totals->loss_sum += sl[0];
    }
}

}  // namespace

size_t head_metrics_workspace(int batch) {
    // per image: the loss (double), then the flags (int32)
    return batch <= 0 ? 0 : ((size_t)batch * 12 + 15) / 16 * 16;
}

hipError_t head_metrics(const int8_t* logits, int batch, int classes, int ld, const int8_t* ascale,
                        const int32_t* labels, int topk, int32_t* pred, double* loss_per_image,
                        niti_eval_totals* totals, void* workspace, size_t workspace_bytes, hipStream_t st) {
    if (!logits || !ascale || !labels || !totals || batch <= 0 || classes <= 0 || ld < classes || topk < 1 ||
        topk > classes || classes > HM_MAXC)
        return hipErrorInvalidValue;
    if (!workspace || workspace_bytes < head_metrics_workspace(batch) || ((uintptr_t)workspace & 7) ||
        ((uintptr_t)totals & 7) || ((uintptr_t)loss_per_image & 7) || ((uintptr_t)pred & 3) || ((uintptr_t)labels & 3))
        return hipErrorInvalidValue;
    double* loss_ws = (double*)workspace;
    int32_t* flag_ws = (int32_t*)(loss_ws + batch);
    const bool vec = ld % 16 == 0 && ((uintptr_t)logits & 15) == 0;
    const dim3 grid((unsigned)((batch + HM_ROWS - 1) / HM_ROWS));
    if (vec)
        hipLaunchKernelGGL(head_metrics_rows_kernel<true>, grid, dim3(256), 0, st, logits, batch, classes, ld, ascale,
                           labels, topk, pred, loss_per_image, loss_ws, flag_ws);
    else
        hipLaunchKernelGGL(head_metrics_rows_kernel<false>, grid, dim3(256), 0, st, logits, batch, classes, ld, ascale,
                           labels, topk, pred, loss_per_image, loss_ws, flag_ws);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(head_metrics_totals_kernel, dim3(1), dim3(256), 0, st, loss_ws, flag_ws, batch, totals);
    return hipGetLastError();
}

}  // namespace niti
