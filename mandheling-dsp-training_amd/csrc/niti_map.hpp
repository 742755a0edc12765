// niti_map.hpp -- grid-stride elementwise launcher used by the layout converters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace niti {

template <class F>
__global__ void map_kernel(int64_t total, F f) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        f(i);
}

template <class F>
inline hipError_t launch_map(int64_t total, F f, hipStream_t st) {
    if (total <= 0) return hipSuccess;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(map_kernel<F>, dim3((unsigned)blocks), dim3(256), 0, st, total, f);
    return hipGetLastError();
}

// Byte fill and copy as plain kernels, for the model steps' captured graphs and the evaluation step.
// On ROCm 7.2 (MI355X) the memset nodes of a captured training step -- the input exponent and the
// range words -- wrote wrong values from the second replay on in some call sequences (a replay
// straight after reading the logits; a replay after a direct-launch evaluation step), while the
// kernel nodes around them replayed correctly.  With these kernels in their place the captured step
// holds kernel nodes only and replays exactly; the evaluation step and the weight hand-over use
// them too, so that they put no memset or copy engine work between two replays.
struct FillBytes {
    uint8_t* p;
    uint8_t v;
    __device__ void operator()(int64_t i) const { p[i] = v; }
};
struct FillWords {
    uint32_t* p;
    uint32_t v;
    __device__ void operator()(int64_t i) const { p[i] = v; }
};
inline hipError_t fill_kernel(void* p, int value, size_t bytes, hipStream_t st) {
    const uint32_t b = (uint32_t)value & 0xffu;
    if (bytes % 4 == 0 && ((uintptr_t)p & 3) == 0)
        return launch_map((int64_t)(bytes / 4), FillWords{(uint32_t*)p, b * 0x01010101u}, st);
    return launch_map((int64_t)bytes, FillBytes{(uint8_t*)p, (uint8_t)b}, st);
}
struct CopyBytes {
    uint8_t* d;
    const uint8_t* s;
    __device__ void operator()(int64_t i) const { d[i] = s[i]; }
};
struct CopyWords {
    uint32_t* d;
    const uint32_t* s;
    __device__ void operator()(int64_t i) const { d[i] = s[i]; }
};
inline hipError_t copy_kernel(void* dst, const void* src, size_t bytes, hipStream_t st) {
    if (bytes % 4 == 0 && (((uintptr_t)dst | (uintptr_t)src) & 3) == 0)
        return launch_map((int64_t)(bytes / 4), CopyWords{(uint32_t*)dst, (const uint32_t*)src}, st);
    return launch_map((int64_t)bytes, CopyBytes{(uint8_t*)dst, (const uint8_t*)src}, st);
}

}  // namespace niti
