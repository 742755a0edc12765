// niti_conv0_wgrad.hip -- the first layer's weight gradient from the pooled gradient and the pool
// codes (conv0_wgrad_codes, niti_kernels.hpp).
//
//   dW0[co][k] = sum over pooled pixels q = (n, py, px) and window elements t = (ty, tx) of
//                (g0[q][co] where bit t of code[q][co] is set, else 0) * xcol[(n, 2 py + ty, 2 px + tx)][k]
//
// The first layer has no input gradient, so its expanded output gradient ([n][oh][ow][cop], three
// quarters zeros behind a 2x2 pool) has one reader: this weight gradient.  It is never written: the
// pooled gradient g0 and the route the forward recorded (pool_code4, one byte per pooled element and
// channel, relu included) carry the same information in half the bytes, and the route becomes a mask
// on the MFMA's A operand.
//
// A step is 64 pooled pixels.  A wave owns whole steps: its g0 and code rows ([64][cop]) and the four
// window elements' xcol rows ([4][64][32]) go through the wave's own 16 KiB of LDS and come back
// K-major by ds_read_b64_tr_b8 (a lane names its own row, so the xcol rows of one window element need
// not be contiguous); the mask is elementwise and is applied after the transposed read.  Per step: 2 K
// halves x 4 window elements x cop / 32 tiles of v_mfma_i32_32x32x32_i8.  The kernel is bound by memory
// latency: every load of a step is issued before any is used, and the next step's before this step's
// LDS traffic.  The waves of a workgroup sum through LDS and the workgroup writes one C-shaped slab
// [cop][32]; splitk_reduce_linear or the update launch's combine sums the slabs.
#include <algorithm>

#include "niti_device.hpp"
#include "niti_kernels.hpp"

namespace niti {

namespace {

constexpr int C0W_STEP = 64;        // pooled pixels per step
constexpr int C0W_WAVES = 4;        // per workgroup
constexpr int C0W_MAX_BLOCKS = 256;  // slabs

struct C0wArgs {
    const int8_t* g0;
    const int8_t* code;
    const int8_t* xcol;
    uint32_t gbytes, xbytes;  // bytes of g0 (= of code) and of xcol
    int pooled;               // n * (oh / 2) * (ow / 2)
    int pw, ow;               // pooled and full row length
    FastDiv fpw;
    int nsteps;
    int32_t* slab;  // [gridDim.x][cop][32]
    uint32_t sbytes;
};

// one step's operands as a wave loads them: 16 bytes per lane per load
template <int COP>
struct C0wStepIn {
    v4i g[COP / 16], c[COP / 16], x[8];
};

// the xcol rows of load i (ty = i >> 2; pooled pixel j = 16 (i & 3) + lane / 4; 16-byte chunk lane & 3 of
// the 64 bytes the pixel's two window elements of that row make): byte offset, or OOB past the batch
__device__ __forceinline__ uint32_t c0w_xoff(const C0wArgs& a, int q0, int i, int lane) {
    const int q = q0 + 16 * (i & 3) + (lane >> 2);
    const uint32_t R = fdiv(a.fpw, (uint32_t)q), px = (uint32_t)q - R * (uint32_t)a.pw;
    const uint32_t row = (2u * R + (uint32_t)(i >> 2)) * (uint32_t)a.ow + 2u * px;
    return q < a.pooled ? row * 32u + 16u * (uint32_t)(lane & 3) : OOB;
}

template <int COP>
__device__ __forceinline__ void c0w_load(const C0wArgs& a, __amdgpu_buffer_rsrc_t rg, __amdgpu_buffer_rsrc_t rc,
                                         __amdgpu_buffer_rsrc_t rx, int step, int lane, C0wStepIn<COP>& in) {
    const bool live = step < a.nsteps;
    const int q0 = step * C0W_STEP;
    // g0 / code rows of the step are contiguous: lane-linear 16-byte chunks (past the end: zeros)
#pragma unroll
    for (int i = 0; i < COP / 16; ++i) {
        const uint32_t off = live ? (uint32_t)q0 * COP + (uint32_t)(i * 64 + lane) * 16u : OOB;
        in.g[i] = buf_load16(rg, off);
        in.c[i] = buf_load16(rc, off);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) in.x[i] = buf_load16(rx, live ? c0w_xoff(a, q0, i, lane) : OOB);
}

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ v4i c0w_tr(const int8_t* p, int row8) {
    const v2i lo = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) v2i*)(p));
    const v2i hi = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) v2i*)(p + row8));
    return v4i{lo[0], lo[1], hi[0], hi[1]};
}

template <int COP>
__global__ void __launch_bounds__(C0W_WAVES * 64) conv0_wgrad_codes_kernel(C0wArgs a) {
    constexpr int TA = COP / 32;                     // co tiles
    constexpr int G_BYTES = C0W_STEP * COP;          // g0 rows of a step (and code rows)
    constexpr int X_BYTES = 4 * C0W_STEP * 32;       // xcol rows [t][pixel][32]
    constexpr int WAVE_BYTES = 2 * G_BYTES + X_BYTES;
    constexpr int RED_BYTES = C0W_WAVES * COP * 32 * 4;
    constexpr int LDS_BYTES = C0W_WAVES * WAVE_BYTES > RED_BYTES ? C0W_WAVES * WAVE_BYTES : RED_BYTES;
    __shared__ __attribute__((aligned(16))) int8_t smem[LDS_BYTES];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int8_t* sg = smem + wid * WAVE_BYTES;
    int8_t* sc = sg + G_BYTES;
    int8_t* sx = sc + G_BYTES;
    const __amdgpu_buffer_rsrc_t rg = make_rsrc(a.g0, a.gbytes), rc = make_rsrc(a.code, a.gbytes);
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.xcol, a.xbytes);

    v16i acc[TA];
#pragma unroll
    for (int t = 0; t < TA; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0;

    // transposed reads: lane 2 q + p of each 16-lane group names row q, 8-byte column p of an 8 x 16
    // byte block, and lane j receives column j of the 8 rows; two reads 8 rows apart are the 16
    // consecutive pixels of this lane's column that the MFMA takes
    const int trow = 16 * (lane >> 5) + ((lane & 15) >> 1);
    const int tcol = 16 * ((lane >> 4) & 1) + 8 * (lane & 1);

    const int stride = (int)gridDim.x * C0W_WAVES;
    int step = (int)blockIdx.x * C0W_WAVES + wid;
    C0wStepIn<COP> cur, nxt;
    c0w_load<COP>(a, rg, rc, rx, step, lane, cur);
    for (; step < a.nsteps; step += stride) {
        c0w_load<COP>(a, rg, rc, rx, step + stride, lane, nxt);  // (past the last step: no memory traffic)
        wave_lds_fence();  // the previous step's reads are done with this wave's LDS
#pragma unroll
        for (int i = 0; i < COP / 16; ++i) {
            *(v4i*)(sg + (i * 64 + lane) * 16) = cur.g[i];
            *(v4i*)(sc + (i * 64 + lane) * 16) = cur.c[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            // chunk lane & 3 = 2 tx + half of pooled pixel j's row ty: window element t = 2 ty + tx
            const int j = 16 * (i & 3) + (lane >> 2), t = 2 * (i >> 2) + ((lane >> 1) & 1);
            *(v4i*)(sx + (t * C0W_STEP + j) * 32 + 16 * (lane & 1)) = cur.x[i];
        }
        wave_lds_fence();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            v4i fx[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) fx[t] = c0w_tr(sx + (t * C0W_STEP + 32 * h + trow) * 32 + tcol, 8 * 32);
#pragma unroll
            for (int ta = 0; ta < TA; ++ta) {
                const int o = (32 * h + trow) * COP + 32 * ta + tcol;
                const v4i g = c0w_tr(sg + o, 8 * COP), c = c0w_tr(sc + o, 8 * COP);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    v4i m;
#pragma unroll
                    for (int k = 0; k < 4; ++k) m[k] = g[k] & (int)pool_code_mask((uint32_t)c[k], t);
                    acc[ta] = __builtin_amdgcn_mfma_i32_32x32x32_i8(m, fx[t], acc[ta], 0, 0, 0);
                }
            }
        }
        cur = nxt;
    }

    // the workgroup's slab: the waves' tiles summed through LDS (C layout [cop][32])
    __syncthreads();
    int32_t* red = (int32_t*)smem;
#pragma unroll
    for (int ta = 0; ta < TA; ++ta)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = 32 * ta + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
            red[(wid * COP + row) * 32 + (lane & 31)] = acc[ta][i];
        }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.slab, a.sbytes);
    for (int e = threadIdx.x; e < COP * 32 / 4; e += C0W_WAVES * 64) {
        v4i s = ((const v4i*)red)[e];
#pragma unroll
        for (int w = 1; w < C0W_WAVES; ++w) s += ((const v4i*)red)[w * (COP * 32 / 4) + e];
        buf_store16(rs, ((uint32_t)blockIdx.x * (COP * 32 / 4) + (uint32_t)e) * 16u, s);
    }
}

int g_c0w_blocks = 0;  // the model path's block count (niti_diag_conv0_wgrad_blocks; 0: the default)

}  // namespace

void diag_conv0_wgrad_blocks(int n) { g_c0w_blocks = n > 0 ? n : 0; }
int conv0_wgrad_codes_model_blocks() { return g_c0w_blocks; }

bool conv0_wgrad_codes_ok(int n, int oh, int ow, int cop, int k) {
    if (n < 1 || oh < 2 || ow < 2 || (oh & 1) || (ow & 1) || (cop != 32 && cop != 64) || k < 1 || k > 32) return false;
    const int64_t px = (int64_t)n * oh * ow;
    // (xcol rows are 32 bytes whatever k; a pooled byte offset one step past the end must fit too)
    return px * 32 <= 0x7fffffff && (px / 4 + C0W_STEP) * cop <= 0x7fffffff;
}

int conv0_wgrad_codes_blocks(int n, int oh, int ow, int blocks) {
    const int64_t pooled = (int64_t)n * (oh / 2) * (ow / 2);
    const int nsteps = (int)((pooled + C0W_STEP - 1) / C0W_STEP);
    if (blocks <= 0) blocks = std::min(C0W_MAX_BLOCKS, (nsteps + C0W_WAVES - 1) / C0W_WAVES);
    return std::max(1, std::min(std::min(blocks, nsteps), C0W_MAX_BLOCKS));
}

hipError_t conv0_wgrad_codes(int n, int oh, int ow, int cop, int k, const int8_t* g0, const int8_t* code,
                             const int8_t* xcol, int blocks, int32_t* slab, size_t slab_bytes, int* slabs,
                             hipStream_t st) {
    if (!conv0_wgrad_codes_ok(n, oh, ow, cop, k) || g0 == nullptr || code == nullptr || xcol == nullptr ||
        slab == nullptr)
        return hipErrorInvalidValue;
    const int grid = conv0_wgrad_codes_blocks(n, oh, ow, blocks);
    if ((size_t)grid * cop * 32 * sizeof(int32_t) > slab_bytes) return hipErrorInvalidValue;
    C0wArgs a{};
    a.g0 = g0;
    a.code = code;
    a.xcol = xcol;
    a.pooled = n * (oh / 2) * (ow / 2);
    a.gbytes = (uint32_t)((int64_t)a.pooled * cop);
    a.xbytes = (uint32_t)((int64_t)n * oh * ow * 32);
    a.pw = ow / 2;
    a.ow = ow;
    a.fpw = make_fastdiv((uint32_t)a.pw);
    a.nsteps = (a.pooled + C0W_STEP - 1) / C0W_STEP;
    a.slab = slab;
    a.sbytes = (uint32_t)((size_t)grid * cop * 32 * sizeof(int32_t));
    if (cop == 64)
        hipLaunchKernelGGL(conv0_wgrad_codes_kernel<64>, dim3((unsigned)grid), dim3(C0W_WAVES * 64), 0, st, a);
    else
        hipLaunchKernelGGL(conv0_wgrad_codes_kernel<32>, dim3((unsigned)grid), dim3(C0W_WAVES * 64), 0, st, a);
    if (slabs != nullptr) *slabs = grid;
    return hipGetLastError();
}

}  // namespace niti
