// niti_conv0.hip -- the first layer's forward pass on its im2col copy (K = 32; niti_quant.hip writes the copy): one
// v_mfma_i32_32x32x32_i8 per 32 pixels x 32 output channels with both operands straight from memory, run twice -- the
// range pass (NITI_RangeEstimate) and the pass that recomputes, requantises by the forward rule of NITI_Conv_Int8.cpp,
// applies relu and the 2x2 max pool (NITI_Maxpool_Int8.cpp) and leaves the pool gradient's route codes.
// conv0_wide_kernel is the general form, conv0_kernel the step's; conv0_ok / conv0_fwd (niti_kernels.hpp) are the
// front.  The layer's weight gradient is niti_conv0_wgrad.hip.
#include <atomic>
#include <type_traits>

#include "niti_device.hpp"
#include "niti_kernels.hpp"
#include "niti_sgd.hpp"

namespace niti {

// ---- first layer on its im2col copy (K = 32) -------------------------------------------------
// y[p][co] = sum_k xcol[p][k] * w[co][k], k < 32: one v_mfma_i32_32x32x32_i8 per 32 pixels x 32
// output channels, both operands straight from memory (a lane's 16-byte fragment is 16
// consecutive k of one row).  Pass 0 publishes max|y| (NITI_RangeEstimate); pass 1 recomputes y
// and requantises it with the forward rule (as requant_quad_kernel), relu, stores the NHWC16
// output and, with pool_out, the 2x2 max pool of the relu'd values.  A wave takes a pair of
// output rows segment by segment (32 pixels of each row), so each pooled pixel's four inputs
// sit in one lane: the x pairs in adjacent accumulator registers, the y pair in the two rows'
// accumulators.  Requires OW % 32 == 0 and OH even (VGG's 32x32 and 224x224 first layers).
struct Conv0 {
    const int8_t* x;  // xcol [P][32]
    const int8_t* w;  // [co][32]
    uint32_t wbytes;
    int co, cop, oh, ow;
    int64_t units;    // (image, row pair, 32-pixel segment)
    uint32_t* amax;   // pass 0 out / pass 1 in
    int8_t* out;      // NHWC16 [P][cop]
    int8_t* pool_out; // [P / 4][cop] or null
    int8_t* pool_c32; // the pooled output as the next layer's C32 input [n][cop/32][oh/2][ow/2][32], or null
    int8_t* out_c32;  // the (unpooled) output as the next layer's C32 input [n][cop/32][oh][ow][32], or null
    int8_t* pool_code; // the pool gradient's route (pool_code4) [P / 4][cop], or null
    const int8_t *exp_in, *wscale;
    int8_t* exp_out;
    int relu;
    // conv0_kernel only: the tensors' sizes for its buffer resources (x; out / out_c32; the pooled
    // three), every one below 2^31 bytes, and the unit decode's divisions
    uint32_t xbytes, obytes, pbytes;
    FastDiv fseg, fpair;
};

// The general form: any cop % 32 == 0 (the weights loaded per tile inside the unit loop) and
// tensors of any size (64-bit addresses), one grid-stride unit after another.  The step's first
// layers (cop <= 64, tensors below 2^31 bytes) run conv0_kernel below instead.
template <int PASS>
__global__ void __launch_bounds__(256) conv0_wide_kernel(Conv0 g) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    const int h = lane >> 5, c = lane & 31;
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(g.w, g.wbytes);
    int s = 2, shift = 0;
    bool raw = false;
    if (PASS == 1) {
        const int bw = __builtin_amdgcn_readfirstlane(bitwidth_of(read_max(g.amax)));
        shift = bw - 7;
        s = shift > 1 ? shift : 2;
        raw = shift <= 0;
        if (blockIdx.x == 0 && threadIdx.x == 0 && g.exp_out != nullptr) {
            const int inc = shift > 1 ? shift : (shift == 1 ? 2 : 0);
            *g.exp_out = (int8_t)((g.exp_in ? (int)*g.exp_in : 0) + (g.wscale ? (int)*g.wscale : 0) + inc);
        }
    }
    const int tiles = g.cop / 32;
    uint32_t m = 0;
    const int segs = g.ow / 32, pairs = g.oh / 2;
    for (int64_t u = wave; u < g.units; u += nwaves) {
        const int seg = (int)(u % segs);
        const int64_t rest = u / segs;
        const int pr = (int)(rest % pairs);
        const int64_t img = rest / pairs;
        const int64_t p0 = (img * g.oh + 2 * pr) * g.ow + seg * 32;  // first pixel of the top row segment
        v4i a[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) a[r] = *(const v4i*)(g.x + (p0 + (int64_t)r * g.ow + c) * 32 + 16 * h);
        for (int t = 0; t < tiles; ++t) {
            const v4i b = buf_load16(rw, (uint32_t)((t * 32 + c) * 32 + 16 * h));
            v16i acc[2];
#pragma unroll
            for (int r = 0; r < 2; ++r)
                acc[r] = __builtin_amdgcn_mfma_i32_32x32x32_i8(b, a[r], v16i{}, 0, 0, 0);
            // acc[r][i]: output channel t * 32 + (i & 3) + 8 (i >> 2) + 4 h, pixel p0 + r * ow + c
            if (PASS == 0) {
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int ch = t * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                        const uint32_t v = ch < g.co ? uabs32(acc[r][i]) : 0u;
                        m = m > v ? m : v;
                    }
            } else {
                int8_t q[2][16];
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        int32_t v;
                        if (raw) {
                            v = (int32_t)(int8_t)acc[r][i];
                        } else if (g.relu) {  // PSTO of max(acc, 0): a negative value is 0 whatever its rounding
                            const uint32_t x = (uint32_t)max(acc[r][i], 0);
                            const uint32_t qp = __builtin_amdgcn_ubfe(x, s >> 1, s - (s >> 1));
                            const uint32_t pr = __builtin_amdgcn_ubfe(x, 0, s >> 1) << (s & 1);
                            v = (int32_t)min((x >> s) + (qp > pr ? 1u : 0u), 127u);
                        } else {
                            v = psto_fast(acc[r][i], s);
                        }
                        if (g.relu && v < 0) v = 0;
                        q[r][i] = (int8_t)v;
                    }
                // lane (pixel c, half h) holds channels 8j + 4h + 0..3 as dword D[j]; one half-wave
                // swap per pair (D0, D2), (D1, D3) gives the lower half channels 0..15 and the
                // upper half 16..31 of its pixel: one 16-byte store per lane and tile
                auto pack = [&](const int8_t* v) {
                    uint32_t d[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        d[j] = (uint32_t)(uint8_t)v[4 * j] | (uint32_t)(uint8_t)v[4 * j + 1] << 8 |
                               (uint32_t)(uint8_t)v[4 * j + 2] << 16 | (uint32_t)(uint8_t)v[4 * j + 3] << 24;
                    const auto x02 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
                    const auto x13 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
                    return v4i{(int)x02[0], (int)x02[1], (int)x13[0], (int)x13[1]};
                };
                v4i qv[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const v4i v = pack(q[r]);
                    qv[r] = v;
                    if (g.out != nullptr) *(v4i*)(g.out + (p0 + (int64_t)r * g.ow + c) * g.cop + t * 32 + 16 * h) = v;
                    if (g.out_c32 != nullptr)
                        *(v4i*)(g.out_c32 + (((img * tiles + t) * g.oh + 2 * pr + r) * (int64_t)g.ow + seg * 32 + c) * 32 +
                                16 * h) = v;
                }
                if (g.pool_out != nullptr) {
                    // vertical max in the lane, horizontal with the neighbour pixel (lane c ^ 1);
                    // even lanes store their pooled pixel
                    int8_t pm[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int v0 = q[0][i] > q[1][i] ? q[0][i] : q[1][i];
                        const int v1 = __shfl_xor(v0, 1, 64);
                        pm[i] = (int8_t)(v0 > v1 ? v0 : v1);
                    }
                    const v4i v = pack(pm);
                    v4i code{0, 0, 0, 0};
                    if (g.pool_code != nullptr) {  // the window: (top, bottom) here, the odd neighbour's
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const uint32_t t1 = (uint32_t)__builtin_amdgcn_mov_dpp(qv[0][k], 0xB1, 0xF, 0xF, false);
                            const uint32_t t3 = (uint32_t)__builtin_amdgcn_mov_dpp(qv[1][k], 0xB1, 0xF, 0xF, false);
                            code[k] = (int)pool_code4((uint32_t)qv[0][k], t1, (uint32_t)qv[1][k], t3, (uint32_t)v[k],
                                                      g.relu != 0);
                        }
                    }
                    if ((c & 1) == 0) {
                        const int64_t pp = (img * (g.oh / 2) + pr) * (g.ow / 2) + seg * 16 + (c >> 1);
                        *(v4i*)(g.pool_out + pp * g.cop + t * 32 + 16 * h) = v;
                        if (g.pool_code != nullptr) *(v4i*)(g.pool_code + pp * g.cop + t * 32 + 16 * h) = code;
                        if (g.pool_c32 != nullptr) {
                            const int64_t hw2 = (int64_t)(g.oh / 2) * (g.ow / 2);
                            *(v4i*)(g.pool_c32 + ((img * tiles + t) * hw2 + pp - img * hw2) * 32 + 16 * h) = v;
                        }
                    }
                }
            }
        }
    }
    if (PASS == 0) {
        m = wave_max(m);
        __shared__ uint32_t red[4];
        if (lane == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) publish_max(g.amax, max(max(red[0], red[1]), max(red[2], red[3])));
    }
}

// The step's form: NT = cop / 32 <= 2 tiles and every tensor below 2^31 bytes (32-bit offsets on
// buffer resources).  A wave walks the units wave, wave + nwaves, ... of a grid the host sizes (any
// size computes the same): the range word, the weights' A fragments and the first unit's pixels
// are loaded together, once per wave, and unit u + 1's pixels are in flight while unit u is
// requantised and stored.  The rule is chosen once per wave from the (uniform) bit width and relu
// flag -- the raw cast, the positive PSTO of a relu layer, the signed PSTO -- and each class runs
// its own straight-line unit loop; the unit's coordinates are wave-uniform (scalar) arithmetic.
template <int PASS, int NT>
__global__ void __launch_bounds__(256) conv0_kernel(Conv0 g) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const uint32_t nwaves = gridDim.x * 4, units = (uint32_t)g.units;
    const int h = lane >> 5, c = lane & 31;
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(g.w, g.wbytes), rx = make_rsrc(g.x, g.xbytes);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(g.out, g.obytes), rc = make_rsrc(g.out_c32, g.obytes);
    const __amdgpu_buffer_rsrc_t rp = make_rsrc(g.pool_out, g.pbytes), rpc = make_rsrc(g.pool_c32, g.pbytes);
    const __amdgpu_buffer_rsrc_t rpk = make_rsrc(g.pool_code, g.pbytes);
    const uint32_t segs = g.fseg.d, pairs = g.fpair.d, ow = (uint32_t)g.ow, oh = (uint32_t)g.oh, cop = NT * 32u;
    uint32_t gm = 0;
    if (PASS == 1) gm = g.amax[lane * MAX_SLOT_STRIDE];
    v4i wa[NT];  // (rows >= co: past the resource, zeros -- their sums are 0)
#pragma unroll
    for (int t = 0; t < NT; ++t) wa[t] = buf_load16(rw, (uint32_t)((t * 32 + c) * 32 + 16 * h));
    const uint32_t lx = (uint32_t)(c * 32 + 16 * h);
    // unit u = (img * pairs + pr) * segs + seg; oh = 2 pairs, so its top row's first pixel is
    // 2 (u / segs) ow + 32 seg.  A unit past the end loads zeros.
    auto xload = [&](uint32_t u, v4i(&a)[2]) {
        const uint32_t q = fdiv(g.fseg, u), seg = u - q * segs;
        const uint32_t o = u < units ? (2u * q * ow + seg * 32u) * 32u + lx : OOB;
        a[0] = buf_load16(rx, o);
        a[1] = buf_load16(rx, o + ow * 32u);
    };
    v4i a[2];
    xload(wave, a);
    int s = 2, cls = 0, lo = -128;
    if (PASS == 1) {
        const int shift = __builtin_amdgcn_readfirstlane(bitwidth_of(wave_max(gm))) - 7;
        s = shift > 1 ? shift : 2;
        cls = shift <= 0 ? 0 : (g.relu ? 1 : 2);
        lo = g.relu ? 0 : -128;
        if (blockIdx.x == 0 && threadIdx.x == 0 && g.exp_out != nullptr) {
            const int inc = shift > 1 ? shift : (shift == 1 ? 2 : 0);
            *g.exp_out = (int8_t)((g.exp_in ? (int)*g.exp_in : 0) + (g.wscale ? (int)*g.wscale : 0) + inc);
        }
    }
    uint32_t m = 0;
    // four values' low bytes as a dword, then lane (pixel c, half h)'s channels 8j + 4h + 0..3 =
    // dword D[j]: one half-wave swap per pair (D0, D2), (D1, D3) gives the lower half channels
    // 0..15 and the upper half 16..31 of its pixel -- one 16-byte store per lane and tile
    auto pack = [&](const int32_t* v) {
        uint32_t d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t p01 = __builtin_amdgcn_perm((uint32_t)v[4 * j + 1], (uint32_t)v[4 * j], 0x0c0c0400u);
            const uint32_t p23 = __builtin_amdgcn_perm((uint32_t)v[4 * j + 3], (uint32_t)v[4 * j + 2], 0x0c0c0400u);
            d[j] = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
        }
        const auto x02 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
        const auto x13 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
        return v4i{(int)x02[0], (int)x02[1], (int)x13[0], (int)x13[1]};
    };
    auto run = [&](auto rule) {
        constexpr int RULE = decltype(rule)::value;  // 0 raw cast, 1 PSTO of max(acc, 0), 2 signed PSTO
        const uint32_t hh = (uint32_t)s >> 1, hs = (uint32_t)s - hh, odd = (uint32_t)s & 1u;
        auto rq = [&](int32_t v) -> int32_t {
            if constexpr (RULE == 0) {
                return max((int32_t)(int8_t)v, lo);
            } else {  // (under relu a negative value is 0 whatever its rounding)
                const uint32_t x = RULE == 1 ? (uint32_t)max(v, 0) : uabs32(v);
                const uint32_t qp = __builtin_amdgcn_ubfe(x, hh, hs), pr = __builtin_amdgcn_ubfe(x, 0, hh) << odd;
                const int32_t r = (int32_t)min((x >> s) + (qp > pr ? 1u : 0u), 127u);
                return RULE == 1 ? r : (v < 0 ? -r : r);
            }
        };
        for (uint32_t u = wave; u < units; u += nwaves) {
            v4i an[2];
            xload(u + nwaves, an);
            const uint32_t q = fdiv(g.fseg, u), seg = u - q * segs;
            const uint32_t img = fdiv(g.fpair, q), pr = q - img * pairs;
            const uint32_t p0 = 2u * q * ow + seg * 32u;           // first pixel of the top row segment
            const uint32_t pp = q * (ow / 2) + seg * 16u + (c >> 1);  // this lane pair's pooled pixel
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                v16i acc[2];
#pragma unroll
                for (int r = 0; r < 2; ++r)
                    acc[r] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wa[t], a[r], v16i{}, 0, 0, 0);
                // acc[r][i]: output channel t * 32 + (i & 3) + 8 (i >> 2) + 4 h, pixel p0 + r * ow + c
                if (PASS == 0) {
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int i = 0; i < 16; ++i) m = max(m, uabs32(acc[r][i]));
                    continue;
                }
                int32_t v[2][16];
                v4i qv[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) v[r][i] = rq(acc[r][i]);
                    qv[r] = pack(v[r]);
                    if (g.out != nullptr) buf_store16(ro, (p0 + r * ow + c) * cop + t * 32 + 16 * h, qv[r]);
                    if (g.out_c32 != nullptr)
                        buf_store16(rc, (((img * NT + t) * oh + 2 * pr + r) * ow + seg * 32u + c) * 32u + 16 * h, qv[r]);
                }
                if (g.pool_out != nullptr) {
                    // vertical max in the lane, horizontal with the neighbour pixel (lane c ^ 1, a
                    // quad_perm move); even lanes store their pooled pixel
                    int32_t pm[16];
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int v0 = max(v[0][i], v[1][i]);
                        pm[i] = max(v0, __builtin_amdgcn_mov_dpp(v0, 0xB1, 0xF, 0xF, false));
                    }
                    const v4i pv = pack(pm);
                    v4i code{0, 0, 0, 0};
                    if (g.pool_code != nullptr) {  // the window: (top, bottom) here, the odd neighbour's
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const uint32_t t1 = (uint32_t)__builtin_amdgcn_mov_dpp(qv[0][k], 0xB1, 0xF, 0xF, false);
                            const uint32_t t3 = (uint32_t)__builtin_amdgcn_mov_dpp(qv[1][k], 0xB1, 0xF, 0xF, false);
                            code[k] = (int)pool_code4((uint32_t)qv[0][k], t1, (uint32_t)qv[1][k], t3, (uint32_t)pv[k],
                                                      g.relu != 0);
                        }
                    }
                    if ((c & 1) == 0) {
                        const uint32_t po = pp * cop + t * 32 + 16 * h;
                        buf_store16(rp, po, pv);
                        if (g.pool_code != nullptr) buf_store16(rpk, po, code);
                        if (g.pool_c32 != nullptr)
                            buf_store16(rpc, (((img * NT + t) * pairs + pr) * (ow / 2) + seg * 16u + (c >> 1)) * 32u + 16 * h, pv);
                    }
                }
            }
            a[0] = an[0];
            a[1] = an[1];
        }
    };
    if (PASS == 0 || cls == 0)
        run(std::integral_constant<int, 0>{});
    else if (cls == 1)
        run(std::integral_constant<int, 1>{});
    else
        run(std::integral_constant<int, 2>{});
    if (PASS == 0) {
        m = wave_max(m);
        __shared__ uint32_t red[4];
        if (lane == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) publish_max(g.amax, max(max(red[0], red[1]), max(red[2], red[3])));
    }
}

// diagnostic: conv0_kernel's grid (niti_diag_conv0_blocks; 0: one resident wave of workgroups)
static std::atomic<int> g_conv0_blocks{0};
void diag_conv0_blocks(int n) { g_conv0_blocks = n > 0 ? n : 0; }

bool conv0_ok(const ConvGeom& g) {
    return g.kh == 1 && g.kw == 1 && g.c_in == 32 && g.cip == 32 && g.ow % 32 == 0 && g.oh % 2 == 0 && g.sh == 1 &&
           g.pt == 0 && g.cop % 32 == 0;
}

hipError_t conv0_fwd(const ConvGeom& g, const int8_t* xcol, const int8_t* w, uint32_t* amax, const ActOut& o,
                     int pass, hipStream_t st, int8_t* pool_c32, int8_t* out_c32, int8_t* pool_code) {
    // (out may be null when the pooled output is kept: pool_out + pool_code carry everything the
    // backward pass reads)
    if (!conv0_ok(g) || o.relu_mask != nullptr) return hipErrorInvalidValue;
    if (o.out == nullptr && (pass == 1 && (o.pool.pool_out == nullptr || pool_code == nullptr))) return hipErrorInvalidValue;
    if ((pool_c32 != nullptr || pool_code != nullptr) && o.pool.pool_out == nullptr) return hipErrorInvalidValue;
    Conv0 k{};
    k.x = xcol;
    k.w = w;
    k.wbytes = (uint32_t)((int64_t)g.c_out * 32);
    k.co = g.c_out;
    k.cop = g.cop;
    k.oh = g.oh;
    k.ow = g.ow;
    k.units = (int64_t)g.n * (g.oh / 2) * (g.ow / 32);
    k.amax = amax;
    k.out = o.out;
    k.pool_out = o.pool.pool_out;
    k.pool_c32 = pool_c32;
    k.out_c32 = out_c32;
    k.pool_code = pool_code;
    k.exp_in = o.exp_in;
    k.wscale = o.wscale;
    k.exp_out = o.exp_out;
    k.relu = o.relu;
    int64_t blocks = (k.units + 3) / 4;
    const int64_t pixels = (int64_t)g.n * g.oh * g.ow;
    if (g.cop > 64 || pixels * 64 >= ((int64_t)1 << 31)) {
        blocks = blocks > 1024 ? 1024 : blocks;
        if (pass == 0)
            hipLaunchKernelGGL(conv0_wide_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, k);
        else
            hipLaunchKernelGGL(conv0_wide_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, k);
        return hipGetLastError();
    }
    k.xbytes = (uint32_t)(pixels * 32);
    k.obytes = (uint32_t)(pixels * g.cop);
    k.pbytes = (uint32_t)(pixels / 4 * g.cop);
    k.fseg = make_fastdiv((uint32_t)(g.ow / 32));
    k.fpair = make_fastdiv((uint32_t)(g.oh / 2));
    using Kern = void (*)(Conv0);
    const Kern f = pass == 0 ? (g.cop == 32 ? conv0_kernel<0, 1> : conv0_kernel<0, 2>)
                             : (g.cop == 32 ? conv0_kernel<1, 1> : conv0_kernel<1, 2>);
    // one resident wave of workgroups, each wave walking its share of the units (speed only)
    const int forced = g_conv0_blocks.load();
    const int res = forced > 0 ? forced : resident_wgs((const void*)f);
    if (res > 0 && blocks > res) blocks = res;
    hipLaunchKernelGGL(f, dim3((unsigned)blocks), dim3(256), 0, st, k);
    return hipGetLastError();
}

}  // namespace niti
