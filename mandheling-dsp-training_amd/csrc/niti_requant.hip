// niti_requant.hip -- the range and requantisation passes over an int32 accumulator tensor: absmax (NITI_RangeEstimate)
// and the power-of-two rescale to int8 (NITI_MNNPstoShiftInt32, CommonOptFunction.cpp:1565-1627) by the forward rule of
// NITI_Conv_Int8.cpp:262-307 -- plain, with relu / the relu-gradient mask, with the 2x2 max pool or its gradient fused
// (requant_quad_kernel), leaving the P16 copy of the output (requant_p16*_kernel), with the 3x3 / 2 stem pool fused
// (requant_pool3_kernel) -- the residual add's requantisation (the rule of niti_resnet.hip), and the weight gradient's
// rule (requant_grad).  The GEMM wrappers of niti_kernels.hip reach these through requant_act(const ActRequant&, ...)
// and the other entry points of niti_kernels.hpp.  (niti_quant.hip is the input image quantiser, a different thing.)
#include <stdlib.h>

#include "niti_device.hpp"
#include "niti_kernels.hpp"
#include "niti_sgd.hpp"

namespace niti {

// =====================================================================================
// Range estimate and requantisation
// =====================================================================================

// max|a| of one range over blocks [0, nb) of the grid (block b of them), published to amax
__device__ __forceinline__ void absmax_body(const int32_t* __restrict__ a, int64_t n, uint32_t* __restrict__ amax,
                                            int64_t b, int64_t nb) {
    uint32_t m = 0;
    const int64_t n4 = n / 4;
    const v4i* a4 = (const v4i*)a;
    for (int64_t i = b * blockDim.x + threadIdx.x; i < n4; i += nb * blockDim.x) {
        const v4i v = a4[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t u = uabs32(v[j]);
            m = m > u ? m : u;
        }
    }
    for (int64_t i = n4 * 4 + b * blockDim.x + threadIdx.x; i < n; i += nb * blockDim.x) {
        const uint32_t u = uabs32(a[i]);
        m = m > u ? m : u;
    }
    m = wave_max(m);
    __shared__ uint32_t red[16];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < (int)(blockDim.x >> 6); ++i) m = m > red[i] ? m : red[i];
        m = m > red[0] ? m : red[0];
        publish_max(amax, m);
    }
}

__global__ void absmax_kernel(const int32_t* __restrict__ a, int64_t n, uint32_t* __restrict__ amax) {
    absmax_body(a, n, amax, blockIdx.x, gridDim.x);
}

// several ranges in one launch: job k owns workgroups [b0_k, b0_{k+1})
__global__ void absmax_many_kernel(AbsmaxJobs J) {
    int k = 0;
    while (k + 1 < J.n && blockIdx.x >= J.j[k + 1].b0) ++k;
    const AbsmaxJob jb = J.j[k];
    const uint32_t end = k + 1 < J.n ? J.j[k + 1].b0 : gridDim.x;
    absmax_body(jb.a, jb.n, jb.amax, blockIdx.x - jb.b0, end - jb.b0);
}

hipError_t absmax_many(const AbsmaxJob* jobs, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (n > ABSMAX_MAX_JOBS) return hipErrorInvalidValue;
    AbsmaxJobs J{};
    uint32_t wg = 0;
    for (int i = 0; i < n; ++i) {
        if (jobs[i].n <= 0) continue;
        int64_t blocks = (jobs[i].n / 4 + 255) / 256;
        if (blocks > 128) blocks = 128;
        if (blocks < 1) blocks = 1;
        J.j[J.n] = jobs[i];
        J.j[J.n++].b0 = wg;
        wg += (uint32_t)blocks;
    }
    if (J.n == 0) return hipSuccess;
    hipLaunchKernelGGL(absmax_many_kernel, dim3(wg), dim3(256), 0, st, J);
    return hipGetLastError();
}

hipError_t absmax_i32(const int32_t* a, int64_t n, uint32_t* amax, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    int64_t blocks = (n / 4 + 255) / 256;
    if (blocks > 512) blocks = 512;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, n, amax);
    return hipGetLastError();
}

// forward / deconv rule, NITI_Conv_Int8.cpp:262-307: shift>1 PSTO(shift); ==1 PSTO(2); else raw cast
// NITI forward shift rule on 16 consecutive channels of one accumulator row
__device__ __forceinline__ v16c requant16(const int32_t* src, bool raw, int s, int relu) {
    const v4i* p = (const v4i*)src;
    v16c q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const v4i v = p[j];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int32_t o = raw ? (int32_t)(int8_t)v[e] : psto_any(v[e], s);
            if (relu && o < 0) o = 0;
            q[j * 4 + e] = (signed char)o;
        }
    }
    return q;
}

__global__ void requant_act_kernel(ActRequant r) {
    const int bw = bitwidth_of(read_max(r.amax));
    const int shift = bw - 7;
    const int s = shift > 1 ? shift : 2;
    const bool raw = shift <= 0;
    const int groups = r.ldc / 16;
    if (blockIdx.x == 0 && threadIdx.x == 0 && r.exp_out != nullptr) {
        const int inc = shift > 1 ? shift : (shift == 1 ? 2 : 0);
        const int ein = r.exp_in ? (int)*r.exp_in : 0;
        const int ws = r.wscale ? (int)*r.wscale : 0;
        *r.exp_out = (int8_t)(ein + ws + inc);
    }
    if (r.pool.pool_out != nullptr || r.pool.dx != nullptr) {
        // one thread per (pooled pixel, 16-channel group)
        const int H = r.pool.H, W = r.pool.W, ph = H / 2, pw = W / 2;
        const int64_t np = r.pool.dx != nullptr ? r.rows : r.rows / 4;  // pooled pixels
        const int64_t total = np * groups;
        for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
             t += (int64_t)gridDim.x * blockDim.x) {
            const int64_t pp = t / groups;
            const int gi = (int)(t - pp * groups);
            const int px = (int)(pp % pw);
            const int64_t rest = pp / pw;
            const int py = (int)(rest % ph);
            const int64_t b = rest / ph;
            const int64_t m0 = (b * H + 2 * py) * W + 2 * px;  // window's first pixel
            const int64_t win[4] = {m0, m0 + 1, m0 + W, m0 + W + 1};
            if (r.pool.pool_out != nullptr) {
                v16c mx;
#pragma unroll
                for (int j = 0; j < 16; ++j) mx[j] = (signed char)-128;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const v16c q = requant16(r.acc + win[k] * r.ldc + gi * 16, raw, s, r.relu);
                    *(v16c*)(r.out_nhwc16 + win[k] * r.ldc + gi * 16) = q;
#pragma unroll
                    for (int j = 0; j < 16; ++j) mx[j] = q[j] > mx[j] ? q[j] : mx[j];
                }
                *(v16c*)(r.pool.pool_out + pp * r.ldc + gi * 16) = mx;
            } else {
                const v16c q = requant16(r.acc + pp * r.ldc + gi * 16, raw, s, 0);
                if (r.out_nhwc16 != nullptr) *(v16c*)(r.out_nhwc16 + pp * r.ldc + gi * 16) = q;
                const v16c mv = *(const v16c*)(r.pool.y + pp * r.ldc + gi * 16);
                unsigned done = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const v16c xv = *(const v16c*)(r.pool.x + win[k] * r.ldc + gi * 16);
                    v16c o;
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const bool take = !((done >> j) & 1u) && xv[j] >= mv[j];
                        if (take) done |= 1u << j;
                        signed char d = take ? q[j] : (signed char)0;
                        if (r.pool.relu && xv[j] <= 0) d = 0;
                        o[j] = d;
                    }
                    *(v16c*)(r.pool.dx + win[k] * r.ldc + gi * 16) = o;
                }
            }
        }
        return;
    }
    const int64_t total = r.rows * groups;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = t / groups;
        const int gi = (int)(t - m * groups);
        const v4i* src = (const v4i*)(r.acc + m * r.ldc + gi * 16);
        v16c q;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const v4i v = src[j];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int32_t o = raw ? (int32_t)(int8_t)v[e] : psto_any(v[e], s);
                if (r.relu && o < 0) o = 0;
                q[j * 4 + e] = (signed char)o;
            }
        }
        if (r.relu_mask != nullptr) {
            const v16c mk = *(const v16c*)(r.relu_mask + m * r.ldc + gi * 16);
#pragma unroll
            for (int j = 0; j < 16; ++j) q[j] = mk[j] > 0 ? q[j] : (signed char)0;
        }
        if (r.out_nhwc16 != nullptr) *(v16c*)(r.out_nhwc16 + m * r.ldc + gi * 16) = q;
        if (r.out_c4 != nullptr) {
            const int64_t b = m / r.hw, p = m - b * r.hw;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int c = gi * 16 + j;
                if (c < r.c_real) r.out_c4[(((int64_t)(c >> 2) * r.n + b) * r.hw + p) * 4 + (c & 3)] = q[j];
            }
        }
    }
}

// Streaming requantisation (the training step's path; out_c4 uses requant_act_kernel above).
// A unit is 4 channels (one 16-byte int32 load, one 4-byte int8 store): consecutive lanes take
// consecutive channel quads, so every wave instruction moves whole contiguous runs (a full
// 1 KiB of accumulator per load), and each thread keeps RQ_U units' loads in flight.
//   RQ_PLAIN     unit over [rows][ldc/4]: out = requant (+relu) (& relu_mask > 0)
//   RQ_POOL_FWD  unit over [pooled pixel][ldc/4]: requant (+relu) the 2x2 window -> out, max -> pool_out
//   RQ_POOL_BWD  unit over [pooled pixel = row][ldc/4]: requant, route to the window's first max
//                of x (relu: and x > 0) in dx, zero elsewhere (+ optional out)
enum { RQ_PLAIN = 0, RQ_POOL_FWD = 1, RQ_POOL_BWD = 2 };
constexpr int RQ_U = 4;

struct RqGeom {
    FastDiv fq, fpw, fph;  // by quads per row, pooled width, pooled height
    int qpr, W;            // quads per row, pre-pool width
    uint32_t units;
    FastDiv fzw, fzh;      // ActRequant::zc_w / zc_h (zero_cls)
};

__device__ __forceinline__ uint32_t rq4(v4i v, bool raw, int s, int relu) {
    uint32_t o = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int32_t q = raw ? (int32_t)(int8_t)v[e] : psto_fast(v[e], s);
        if (relu && q < 0) q = 0;
        o |= ((uint32_t)q & 0xffu) << (8 * e);
    }
    return o;
}
__device__ __forceinline__ uint32_t bmax4(uint32_t a, uint32_t b) {
    uint32_t o = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int x = (int8_t)(a >> (8 * e)), y = (int8_t)(b >> (8 * e));
        o |= ((uint32_t)(x > y ? x : y) & 0xffu) << (8 * e);
    }
    return o;
}

template <int MODE>
__global__ void __launch_bounds__(256) requant_quad_kernel(ActRequant r, RqGeom g) {
    const int bw = bitwidth_of(read_max(r.amax));  // whole wave active
    const int shift = bw - 7;
    const int s = shift > 1 ? shift : 2;
    const bool raw = shift <= 0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && r.exp_out != nullptr) {
        const int inc = shift > 1 ? shift : (shift == 1 ? 2 : 0);
        const int ein = r.exp_in ? (int)*r.exp_in : 0;
        const int ws = r.wscale ? (int)*r.wscale : 0;
        *r.exp_out = (int8_t)(ein + ws + inc);
    }
    const uint32_t stride = gridDim.x * 256u;
    const int ldc = r.ldc;
    for (uint32_t u0 = blockIdx.x * 256u + threadIdx.x; u0 < g.units; u0 += stride * RQ_U) {
        if (MODE == RQ_PLAIN) {
            v4i v[RQ_U];
            uint32_t mk[RQ_U];
#pragma unroll
            for (int j = 0; j < RQ_U; ++j) {
                const uint32_t u = u0 + j * stride;
                bool ld = u < g.units;
                if (ld && r.zero_cls != 0) {  // a tap-less sub-pixel class: 0, its accumulators unread
                    const uint32_t row = fdiv(g.fq, u), t = fdiv(g.fzw, row);
                    const uint32_t x = row - t * g.fzw.d, y = t - fdiv(g.fzh, t) * g.fzh.d;
                    ld = !((r.zero_cls >> (2 * (y & 1u) + (x & 1u))) & 1);
                }
                v[j] = ld ? __builtin_nontemporal_load((const v4i*)r.acc + u) : v4i{0, 0, 0, 0};
                mk[j] = (r.relu_mask != nullptr && u < g.units) ? ((const uint32_t*)r.relu_mask)[u] : 0x01010101u;
            }
#pragma unroll
            for (int j = 0; j < RQ_U; ++j) {
                const uint32_t u = u0 + j * stride;
                if (u >= g.units) break;
                uint32_t o = rq4(v[j], raw, s, r.relu);
                if (r.relu_mask != nullptr) {
                    uint32_t keep = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if ((int8_t)(mk[j] >> (8 * e)) > 0) keep |= 0xffu << (8 * e);
                    o &= keep;
                }
                ((uint32_t*)r.out_nhwc16)[u] = o;
            }
        } else {
            // window rows of each unit
            int64_t wrow[RQ_U];
            uint32_t pp_[RQ_U], img_[RQ_U];
            int cq_[RQ_U];
#pragma unroll
            for (int j = 0; j < RQ_U; ++j) {
                const uint32_t u = u0 + j * stride;
                const uint32_t uu = u < g.units ? u : 0u;
                const uint32_t pp = fdiv(g.fq, uu);
                cq_[j] = (int)(uu - pp * (uint32_t)g.qpr);
                const uint32_t rest = fdiv(g.fpw, pp);
                const int px = (int)(pp - rest * g.fpw.d);
                const uint32_t b = fdiv(g.fph, rest);
                const int py = (int)(rest - b * g.fph.d);
                wrow[j] = ((int64_t)b * (2 * g.fph.d) + 2 * py) * g.W + 2 * px;
                pp_[j] = pp;
                img_[j] = b;
            }
            if (MODE == RQ_POOL_FWD) {
                v4i v[RQ_U][4];
#pragma unroll
                for (int j = 0; j < RQ_U; ++j)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int64_t row = wrow[j] + (k & 1) + (k >> 1) * g.W;
                        v[j][k] = u0 + j * stride < g.units
                                      ? __builtin_nontemporal_load((const v4i*)(r.acc + row * ldc) + cq_[j])
                                      : v4i{0, 0, 0, 0};
                    }
#pragma unroll
                for (int j = 0; j < RQ_U; ++j) {
                    if (u0 + j * stride >= g.units) break;
                    uint32_t mx = 0x80808080u;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int64_t row = wrow[j] + (k & 1) + (k >> 1) * g.W;
                        const uint32_t o = rq4(v[j][k], raw, s, r.relu);
                        ((uint32_t*)(r.out_nhwc16 + row * ldc))[cq_[j]] = o;
                        mx = bmax4(mx, o);
                    }
                    ((uint32_t*)(r.pool.pool_out + (int64_t)pp_[j] * ldc))[cq_[j]] = mx;
                }
            } else {
                v4i v[RQ_U];
                uint32_t yv[RQ_U], xv[RQ_U][4];
#pragma unroll
                for (int j = 0; j < RQ_U; ++j) {
                    const bool ok = u0 + j * stride < g.units;
                    v[j] = ok ? __builtin_nontemporal_load((const v4i*)(r.acc + (int64_t)pp_[j] * ldc) + cq_[j])
                              : v4i{0, 0, 0, 0};
                    yv[j] = ok ? ((const uint32_t*)(r.pool.y + (int64_t)pp_[j] * ldc))[cq_[j]] : 0u;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int64_t row = wrow[j] + (k & 1) + (k >> 1) * g.W;
                        xv[j][k] = ok ? ((const uint32_t*)(r.pool.x + row * ldc))[cq_[j]] : 0u;
                    }
                }
#pragma unroll
                for (int j = 0; j < RQ_U; ++j) {
                    if (u0 + j * stride >= g.units) break;
                    const uint32_t q = rq4(v[j], raw, s, 0);
                    if (r.out_nhwc16 != nullptr) ((uint32_t*)(r.out_nhwc16 + (int64_t)pp_[j] * ldc))[cq_[j]] = q;
                    uint32_t done = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        uint32_t o = 0;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int x = (int8_t)(xv[j][k] >> (8 * e)), m = (int8_t)(yv[j] >> (8 * e));
                            const bool take = !((done >> e) & 1u) && x >= m;
                            if (take) done |= 1u << e;
                            if (take && !(r.pool.relu && x <= 0)) o |= q & (0xffu << (8 * e));
                        }
                        const int64_t row = wrow[j] + (k & 1) + (k >> 1) * g.W;
                        ((uint32_t*)(r.pool.dx + row * ldc))[cq_[j]] = o;
                        if (r.pool.dx_c32 != nullptr) {  // [img][c / 32][H][W][32]: 4 channels of one pixel
                            const int64_t hw = (int64_t)(2 * g.fph.d) * g.W;
                            const int64_t pix = row - (int64_t)img_[j] * hw;
                            const int c = 4 * cq_[j];
                            *(uint32_t*)(r.pool.dx_c32 + (((int64_t)img_[j] * (ldc / 32) + c / 32) * hw + pix) * 32 + (c & 31)) = o;
                        }
                    }
                }
            }
        }
    }
}

// Requantisation passes that also leave the P16 copy ([pixels/16][ldc][16], niti_wgrad.hip) of
// their output, so the input-gradient chain hands dy to the P16 weight gradient without a layout
// launch of its own.  A thread takes one channel quad of a run of output pixels covering whole
// 16-pixel blocks -- G pooled pixels whose 2x2 windows are 4G consecutive dx pixels (G = 4: a pooled row of an 8x8 image, one 4x4 image, four 2x2 images;
// G = 8: a pooled row of a 16x16 image).  It computes and stores the NHWC16 output exactly as
// requant_quad_kernel does, then transposes each 4 pixels x 4 channels in registers (v_perm) and
// writes every block's 4 channels x 16 pixels as 64 contiguous bytes (consecutive lanes,
// consecutive quads: a wave stores whole 4 KiB runs).
template <int W>
__host__ __device__ constexpr int p16_group() { return W == 16 ? 8 : 4; }
// position, inside the run, of corner k (0: top left, 1: top right, 2, 3: bottom) of pooled pixel j
template <int W>
__device__ constexpr int p16_loc(int j, int k) {
    if constexpr (W >= 8) return (k >> 1) * W + 2 * j + (k & 1);               // one pooled row
    else if constexpr (W == 4) return (2 * (j >> 1) + (k >> 1)) * 4 + 2 * (j & 1) + (k & 1);  // one image
    else return 4 * j + 2 * (k >> 1) + (k & 1);                                  // four 2x2 images
}

template <int MODE, int W>
__global__ void __launch_bounds__(256) requant_p16_kernel(ActRequant r, RqGeom g) {
    static_assert(MODE == RQ_POOL_BWD, "the plain pass is requant_p16_plain_kernel");
    constexpr int G = p16_group<W>();  // pooled pixels per thread
    constexpr int NPX = 4 * G;         // dx pixels per thread
    const int bw = bitwidth_of(read_max(r.amax));
    const int shift = bw - 7;
    const int s = shift > 1 ? shift : 2;
    const bool raw = shift <= 0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && r.exp_out != nullptr) {
        const int inc = shift > 1 ? shift : (shift == 1 ? 2 : 0);
        const int ein = r.exp_in ? (int)*r.exp_in : 0;
        const int ws = r.wscale ? (int)*r.wscale : 0;
        *r.exp_out = (int8_t)(ein + ws + inc);
    }
    const int ldc = r.ldc;
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < g.units; u += gridDim.x * 256u) {
        const uint32_t grp = fdiv(g.fq, u);
        const int cq = (int)(u - grp * (uint32_t)g.qpr);
        const int64_t d0 = (int64_t)grp * NPX;  // the run's first output pixel
        uint32_t d[NPX];
        {
            const int64_t p0 = (int64_t)grp * G;  // the run's first pooled pixel
            v4i v[G];
            uint32_t yv[G], xv[G][4];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                v[j] = __builtin_nontemporal_load((const v4i*)(r.acc + (p0 + j) * ldc) + cq);
                yv[j] = ((const uint32_t*)(r.pool.y + (p0 + j) * ldc))[cq];
#pragma unroll
                for (int k = 0; k < 4; ++k) xv[j][k] = ((const uint32_t*)(r.pool.x + (d0 + p16_loc<W>(j, k)) * ldc))[cq];
            }
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const uint32_t q = rq4(v[j], raw, s, 0);
                if (r.out_nhwc16 != nullptr) ((uint32_t*)(r.out_nhwc16 + (p0 + j) * ldc))[cq] = q;
                uint32_t done = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t o = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int x = (int8_t)(xv[j][k] >> (8 * e)), m = (int8_t)(yv[j] >> (8 * e));
                        const bool take = !((done >> e) & 1u) && x >= m;
                        if (take) done |= 1u << e;
                        if (take && !(r.pool.relu && x <= 0)) o |= q & (0xffu << (8 * e));
                    }
                    ((uint32_t*)(r.pool.dx + (d0 + p16_loc<W>(j, k)) * ldc))[cq] = o;
                    d[p16_loc<W>(j, k)] = o;
                }
            }
        }
#pragma unroll
        for (int b = 0; b < NPX / 16; ++b) {
            v4i c[4];  // channel e: the block's 16 pixels
#pragma unroll
            for (int t = 0; t < 4; ++t) {  // 4x4 byte transpose of pixels 16b + 4t .. 4t + 3
                const uint32_t a0 = d[16 * b + 4 * t], a1 = d[16 * b + 4 * t + 1], a2 = d[16 * b + 4 * t + 2],
                               a3 = d[16 * b + 4 * t + 3];
                const uint32_t t0 = __builtin_amdgcn_perm(a1, a0, 0x05010400u);  // a0.0 a1.0 a0.1 a1.1
                const uint32_t t1 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);  // a0.2 a1.2 a0.3 a1.3
                const uint32_t t2 = __builtin_amdgcn_perm(a3, a2, 0x05010400u);
                const uint32_t t3 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
                c[0][t] = (int)__builtin_amdgcn_perm(t2, t0, 0x05040100u);
                c[1][t] = (int)__builtin_amdgcn_perm(t2, t0, 0x07060302u);
                c[2][t] = (int)__builtin_amdgcn_perm(t3, t1, 0x05040100u);
                c[3][t] = (int)__builtin_amdgcn_perm(t3, t1, 0x07060302u);
            }
            int8_t* o = r.out_p16 + ((d0 / 16 + b) * ldc + 4 * cq) * 16;
#pragma unroll
            for (int e = 0; e < 4; ++e) *(v4i*)(o + 16 * e) = c[e];
        }
    }
}

// The plain pass with 4 rows per thread (4x the threads of the 16-row form above, which ran
// latency-bound at one block per CU): lanes 4 cq + sub take rows 4 sub .. 4 sub + 3 of a 16-row
// block and channel quad cq, so the four lanes of a quad write each channel's 16 P16 bytes as
// four adjacent dwords.
__global__ void __launch_bounds__(256) requant_p16_plain_kernel(ActRequant r, RqGeom g) {
    const int bw = bitwidth_of(read_max(r.amax));
    const int shift = bw - 7;
    const int s = shift > 1 ? shift : 2;
    const bool raw = shift <= 0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && r.exp_out != nullptr) {
        const int inc = shift > 1 ? shift : (shift == 1 ? 2 : 0);
        const int ein = r.exp_in ? (int)*r.exp_in : 0;
        const int ws = r.wscale ? (int)*r.wscale : 0;
        *r.exp_out = (int8_t)(ein + ws + inc);
    }
    const int ldc = r.ldc;
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < g.units; u += gridDim.x * 256u) {
        const int sub = (int)(u & 3u);
        const uint32_t qu = u >> 2;
        const uint32_t blk = fdiv(g.fq, qu);
        const int cq = (int)(qu - blk * (uint32_t)g.qpr);
        const int64_t row0 = (int64_t)blk * 16 + 4 * sub;
        v4i v[4];
        uint32_t mk[4], d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = __builtin_nontemporal_load((const v4i*)(r.acc + (row0 + i) * ldc) + cq);
            mk[i] = r.relu_mask != nullptr ? ((const uint32_t*)(r.relu_mask + (row0 + i) * ldc))[cq] : 0x01010101u;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t o = rq4(v[i], raw, s, r.relu);
            if (r.relu_mask != nullptr) {
                uint32_t keep = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((int8_t)(mk[i] >> (8 * e)) > 0) keep |= 0xffu << (8 * e);
                o &= keep;
            }
            ((uint32_t*)(r.out_nhwc16 + (row0 + i) * ldc))[cq] = o;
            d[i] = o;
        }
        const uint32_t t0 = __builtin_amdgcn_perm(d[1], d[0], 0x05010400u);
        const uint32_t t1 = __builtin_amdgcn_perm(d[1], d[0], 0x07030602u);
        const uint32_t t2 = __builtin_amdgcn_perm(d[3], d[2], 0x05010400u);
        const uint32_t t3 = __builtin_amdgcn_perm(d[3], d[2], 0x07030602u);
        uint32_t* o = (uint32_t*)(r.out_p16 + ((int64_t)blk * ldc + 4 * cq) * 16) + sub;
        o[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u);
        o[4] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
        o[8] = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
        o[12] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
    }
}

template <int MODE>
static void launch_requant_p16(const ActRequant& r, RqGeom g, int64_t blocks, hipStream_t st) {
    switch (r.pool.W) {
        case 2: hipLaunchKernelGGL((requant_p16_kernel<RQ_POOL_BWD, 2>), dim3((unsigned)blocks), dim3(256), 0, st, r, g); break;
        case 4: hipLaunchKernelGGL((requant_p16_kernel<RQ_POOL_BWD, 4>), dim3((unsigned)blocks), dim3(256), 0, st, r, g); break;
        case 8: hipLaunchKernelGGL((requant_p16_kernel<RQ_POOL_BWD, 8>), dim3((unsigned)blocks), dim3(256), 0, st, r, g); break;
        default: hipLaunchKernelGGL((requant_p16_kernel<RQ_POOL_BWD, 16>), dim3((unsigned)blocks), dim3(256), 0, st, r, g); break;
    }
}

bool requant_p16_ok(const ActRequant& r) {
    if (r.ldc % 16 != 0 || r.out_c4 != nullptr || r.pool.pool_out != nullptr) return false;
    if (r.pool.dx == nullptr) return r.out_nhwc16 != nullptr && r.rows % 16 == 0;
    const int W = r.pool.W;
    if (r.pool.H != W || !(W == 2 || W == 4 || W == 8 || W == 16)) return false;
    const int gsz = W == 16 ? p16_group<16>() : p16_group<8>();
    return r.rows % gsz == 0;
}

// Residual add fused with its requantisation (the rule of niti_resnet.hip): the range comes from a
// residual_add pass that stores no z (and, data parallel, a MAX all-reduce); this pass recomputes z
// from the int8 operands and applies the forward rule exactly as requant_act (RQ_PLAIN) on z:
// out = relu?(PSTO(z, shift) | (int8) z), *ez = e_hi - d, *exp_out = *ez + inc.
__global__ void __launch_bounds__(256) residual_requant_kernel(const int8_t* __restrict__ a, const int8_t* __restrict__ ea,
                                                               const int8_t* __restrict__ b, const int8_t* __restrict__ eb,
                                                               int64_t n16, const uint32_t* __restrict__ amax,
                                                               int8_t* __restrict__ ez, int8_t* __restrict__ exp_out,
                                                               int relu, const int8_t* __restrict__ relu_mask,
                                                               int8_t* __restrict__ out, int spec,
                                                               uint32_t* __restrict__ hint, int pk) {
    const int xa = *ea, xb = *eb;
    const bool a_hi = xa >= xb;
    const int diff = a_hi ? xa - xb : xb - xa;
    const int d = diff < 23 ? diff : 23, r = diff - d;
    int bw;
    if (spec == 1) {  // launch A: the guess; the range is published below
        bw = (int)spec_pick(hint, relu ? (a_hi ? xa : xb) - d : 0) - 1;  // forward: on z's scale
        if (bw < 0) bw = 0;  // (no hint yet: B redoes unless the max is 0)
        if (blockIdx.x == 0 && threadIdx.x == 0)
            __hip_atomic_store(hint + 1, (uint32_t)bw + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        bw = bitwidth_of(read_max(amax));  // whole wave active
        if (spec == 2) {  // launch B: A's output stands unless the (all-reduced) range differs
            const int used = __builtin_amdgcn_readfirstlane(
                                 (int)__hip_atomic_load(hint + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) - 1;
            if (blockIdx.x == 0 && threadIdx.x < 64) spec_learn(hint, bw, relu ? (a_hi ? xa : xb) - d : 0, threadIdx.x);
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                if (bw != used) __hip_atomic_fetch_add(hint + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int shift = bw - 7;
                const int e_z = (a_hi ? xa : xb) - d;
                if (ez != nullptr) *ez = (int8_t)e_z;
                if (exp_out != nullptr) *exp_out = (int8_t)(e_z + (shift > 1 ? shift : (shift == 1 ? 2 : 0)));
            }
            if (bw == used) return;
        }
    }
    const int shift = bw - 7;
    const int s = shift > 1 ? shift : 2;
    const bool raw = shift <= 0;
    if (spec == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
        const int e_z = (a_hi ? xa : xb) - d;
        if (ez != nullptr) *ez = (int8_t)e_z;
        if (exp_out != nullptr) *exp_out = (int8_t)(e_z + (shift > 1 ? shift : (shift == 1 ? 2 : 0)));
    }
    uint32_t m = 0;
    if (pk && !raw) {  // the bit-field form (res_rule4)
        const ResRule k = res_rule(d, r, s);
        const int8_t* hi = a_hi ? a : b;
        const int8_t* lo = a_hi ? b : a;
        int mx = 0, mn = 0;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
            const v4i vh = ((const v4i*)hi)[i], vl = ((const v4i*)lo)[i];
            v4i mk;
            if (relu_mask != nullptr) mk = ((const v4i*)relu_mask)[i];
            v4i q;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                uint32_t o = relu ? res_rule4<true>((uint32_t)vh[w], (uint32_t)vl[w], k, mx, mn, spec == 1)
                                  : res_rule4<false>((uint32_t)vh[w], (uint32_t)vl[w], k, mx, mn, spec == 1);
                if (relu_mask != nullptr) o &= sw_expand(sw_pos_hi((uint32_t)mk[w]));
                q[w] = (int)o;
            }
            ((v4i*)out)[i] = q;
        }
        m = max(uabs32(mx), uabs32(mn));
    } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
        const v16c va = ((const v16c*)a)[i], vb = ((const v16c*)b)[i];
        v16c mk;
        if (relu_mask != nullptr) mk = ((const v16c*)relu_mask)[i];
        v16c q;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int32_t z = residual_z(a_hi ? va[e] : vb[e], a_hi ? vb[e] : va[e], d, r);
            if (spec == 1) {
                const uint32_t u = uabs32(z);
                m = m > u ? m : u;
            }
            int32_t o = raw ? (int32_t)(int8_t)z : psto_fast(z, s);
            if (relu && o < 0) o = 0;
            if (relu_mask != nullptr && mk[e] <= 0) o = 0;  // the next op's NITI_ReluGrad_Int8, fused
            q[e] = (signed char)o;
        }
        ((v16c*)out)[i] = q;
    }
    }
    if (spec == 1) {  // NITI_RangeEstimate of z for launch B
        m = wave_max(m);
        __shared__ uint32_t red[4];
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) publish_max(const_cast<uint32_t*>(amax), max(max(red[0], red[1]), max(red[2], red[3])));
    }
}

hipError_t residual_requant(const int8_t* a, const int8_t* ea, const int8_t* b, const int8_t* eb, int64_t n,
                            const uint32_t* amax, int8_t* ez, int8_t* exp_out, int relu, int8_t* out, hipStream_t st,
                            const int8_t* relu_mask, int spec, uint32_t* slot) {
    if (n < 0 || n % 16 != 0 || !a || !b || !ea || !eb || !amax || !out) return hipErrorInvalidValue;
    if (spec < 0 || spec > 2 || (spec != 0 && slot == nullptr)) return hipErrorInvalidValue;
    const int64_t n16 = n / 16;
    int64_t blocks = (n16 + 255) / 256;
    blocks = blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks;
    // NITI_RES_PK=0: the 32-bit loop only (an A/B switch for the packed form)
    static const int pk = getenv("NITI_RES_PK") ? atoi(getenv("NITI_RES_PK")) : 1;
    hipLaunchKernelGGL(residual_requant_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, ea, b, eb, n16, amax, ez,
                       exp_out, relu, relu_mask, out, spec, slot, pk);
    return hipGetLastError();
}

// The requantisation with the 3x3 / 2 (pad 1) max pool fused (ActRequant::pool3, ResNet-18's
// stem: NITI_Conv_Int8.cpp:266-307's rescale + relu, then NITI_Maxpool_Int8.cpp:24-72 over the
// int8 result, first maximum in (ky, kx) order), so the pre-pool int8 image is neither written
// (unless out_nhwc16) nor read back by a pool pass.  One thread per pooled column strip of
// RQ3_ROWS pooled rows and 4 channels: each step requantises the two new input rows' three
// columns and carries the last one down as the next window's top row, so the accumulators are
// read once vertically (plus one row per strip); the horizontal overlap (the shared column of
// neighbouring windows) is the neighbouring lanes' load of the same lines.  VALU-bound before
// the relu forms below (~700 operations per pooled quad: 160 us for the batch-128 stem).
constexpr int RQ3_ROWS = 4;  // (2-28 measured: 103-113 us, profiles/r05_stem_pool.txt)
struct Rq3Geom {
    FastDiv fq, fow, fch;  // by quads per row, pooled width, strips per image
    int qpr, H, W, OH, rows;  // rows: pooled rows per strip
    uint32_t units;
    int remap;  // one thread per unit, blocks XCD-remapped (else grid-stride)
};
__device__ __forceinline__ void pool3_take(uint32_t o, int k, uint32_t& m, uint32_t& a) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int ov = (int8_t)(o >> (8 * e)), mv = (int8_t)(m >> (8 * e)), av = (int8_t)(a >> (8 * e));
        if (av < 0 || ov > mv) {
            m = (m & ~(0xffu << (8 * e))) | (o & (0xffu << (8 * e)));
            a = (a & ~(0xffu << (8 * e))) | ((uint32_t)k << (8 * e));
        }
    }
}
// relu(PSTO(v, s)) of four accumulators, packed (rq4 with relu and s >= 2, in fewer VALU
// operations: a <= 0 gives 0 either way, so the sign paths go; the pool is VALU-bound otherwise)
__device__ __forceinline__ uint32_t rq4_relu(v4i v, int s) {
    const int h = s >> 1, odd = s & 1;
    uint32_t o = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t x = (uint32_t)max(v[e], 0);
        const uint32_t qp = __builtin_amdgcn_ubfe(x, h, s - h), pr = __builtin_amdgcn_ubfe(x, 0, h) << odd;
        const uint32_t q = min((x >> s) + (qp > pr ? 1u : 0u), 127u);
        o |= q << (8 * e);
    }
    return o;
}
// pool3_take for bytes in [0, 127] (relu outputs), four at once: where o > m (strict: the first
// maximum stays), m = o and a = k
__device__ __forceinline__ void pool3_take_u7(uint32_t o, uint32_t k4, uint32_t& m, uint32_t& a) {
    const uint32_t gt = ((o | 0x80808080u) - m - 0x01010101u) & 0x80808080u;  // bytes: 127 + o - m >= 128
    const uint32_t mask = (gt >> 7) * 0xffu;
    m = (m & ~mask) | (o & mask);
    a = (a & ~mask) | (k4 & mask);
}

template <bool RELU>
__global__ void __launch_bounds__(256) requant_pool3_kernel(ActRequant r, Rq3Geom g) {
    // (wave-uniform: scalar branches below)
    const int bw = __builtin_amdgcn_readfirstlane(bitwidth_of(read_max(r.amax)));
    const int shift = bw - 7;
    const int s = shift > 1 ? shift : 2;
    const bool raw = shift <= 0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && r.exp_out != nullptr) {
        const int inc = shift > 1 ? shift : (shift == 1 ? 2 : 0);
        const int ein = r.exp_in ? (int)*r.exp_in : 0;
        const int ws = r.wscale ? (int)*r.wscale : 0;
        *r.exp_out = (int8_t)(ein + ws + inc);
    }
    const uint32_t qpr = (uint32_t)g.qpr;
    const int OW = (int)g.fow.d;
    const int64_t RS = (int64_t)g.W * qpr;  // input row stride, quads
    const uint32_t bid = g.remap ? (uint32_t)xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
    auto rq = [&](const v4i& v) { return RELU && !raw ? rq4_relu(v, s) : rq4(v, raw, s, RELU); };
    auto take = [&](uint32_t o, int k, uint32_t& m, uint32_t& a) {
        if (RELU)
            pool3_take_u7(o, 0x01010101u * (uint32_t)k, m, a);
        else
            pool3_take(o, k, m, a);
    };
    for (uint32_t u = bid * 256u + threadIdx.x; u < g.units; u += g.remap ? g.units : gridDim.x * 256u) {
        const uint32_t pix = fdiv(g.fq, u), q = u - pix * qpr;
        const uint32_t t = fdiv(g.fow, pix), ox = pix - t * g.fow.d;
        const uint32_t b = fdiv(g.fch, t), ch = t - b * g.fch.d;
        const int oy0 = (int)ch * g.rows, oy1 = min(g.OH, oy0 + g.rows);
        const int x0 = 2 * (int)ox - 1;
        const bool c0 = x0 >= 0, c2 = x0 + 2 < g.W;
        // columns x0, x0 + 1, x0 + 2 of a row as offsets from column x0 + 1 (a column outside the
        // image reads column x0 + 1 instead: loaded, never taken)
        const int64_t o0 = c0 ? -(int64_t)qpr : 0, o2 = c2 ? (int64_t)qpr : 0;
        const v4i* p = (const v4i*)r.acc + ((int64_t)b * g.H * g.W + 2 * oy0 * g.W + x0 + 1) * qpr + q;
        uint32_t* y0 = r.out_nhwc16 ? (uint32_t*)r.out_nhwc16 + (p - (const v4i*)r.acc) : nullptr;
        // the two input rows 2 oy, 2 oy + 1 at p (the second: the first again past the image)
        auto load = [&](const v4i* p, int oy, v4i* a) {
            const v4i* p1 = 2 * oy + 1 < g.H ? p + RS : p;
            a[0] = p[o0];
            a[1] = p[0];
            a[2] = p[o2];
            a[3] = p1[o0];
            a[4] = p1[0];
            a[5] = p1[o2];
        };
        uint32_t top[3] = {0, 0, 0};
        if (oy0 > 0) {
            const v4i* pt = p - RS;
            top[0] = rq(pt[o0]);
            top[1] = rq(pt[0]);
            top[2] = rq(pt[o2]);
        }
        auto step = [&](const v4i* a, int oy) {
            const bool r2 = 2 * oy + 1 < g.H;
            uint32_t mid[3], bot[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                mid[k] = rq(a[k]);
                bot[k] = rq(a[3 + k]);
            }
            // bytes: max, position.  With relu every value is >= 0: start from 0 at the window's
            // first position, later positions taken where strictly greater (the first maximum)
            uint32_t m = RELU ? 0u : 0x80808080u;
            uint32_t am = RELU ? 0x01010101u * (uint32_t)((oy > 0 ? 0 : 3) + (c0 ? 0 : 1)) : 0xffffffffu;
            if (oy > 0) {
                if (c0) take(top[0], 0, m, am);
                take(top[1], 1, m, am);
                if (c2) take(top[2], 2, m, am);
            }
            if (c0) take(mid[0], 3, m, am);
            take(mid[1], 4, m, am);
            if (c2) take(mid[2], 5, m, am);
            if (r2) {
                if (c0) take(bot[0], 6, m, am);
                take(bot[1], 7, m, am);
                if (c2) take(bot[2], 8, m, am);
            }
            const int64_t po = (((int64_t)b * g.OH + oy) * OW + ox) * qpr + q;
            ((uint32_t*)r.pool3.out)[po] = m;
            ((uint32_t*)r.pool3.arg)[po] = am;
            if (y0 != nullptr) {  // each pre-pool pixel once: rows 2 oy, 2 oy + 1 x columns x0 + 1, x0 + 2
                uint32_t* d = y0 + (int64_t)(oy - oy0) * 2 * RS;
                d[0] = mid[1];
                if (c2) d[qpr] = mid[2];
                if (r2) {
                    d[RS] = bot[1];
                    if (c2) d[RS + qpr] = bot[2];
                }
            }
            top[0] = bot[0];
            top[1] = bot[1];
            top[2] = bot[2];
        };
        // two register sets, each step's rows loaded one step ahead
        v4i A[6], B[6];
        load(p, oy0, A);
        for (int oy = oy0;;) {
            if (oy + 1 < oy1) load(p + 2 * RS, oy + 1, B);
            step(A, oy);
            if (++oy >= oy1) break;
            p += 2 * RS;
            if (oy + 1 < oy1) load(p + 2 * RS, oy + 1, A);
            step(B, oy);
            if (++oy >= oy1) break;
            p += 2 * RS;
        }
    }
}

hipError_t requant_act(const ActRequant& r, hipStream_t st) {
    if (r.ldc % 16 != 0 || r.acc == nullptr || r.amax == nullptr) return hipErrorInvalidValue;
    if (r.pool.pool_out != nullptr || r.pool.dx != nullptr) {
        if (r.pool.H % 2 || r.pool.W % 2 || r.pool.H <= 0 || r.pool.W <= 0) return hipErrorInvalidValue;
        if (r.pool.pool_out != nullptr && (r.out_nhwc16 == nullptr || r.rows % ((int64_t)r.pool.H * r.pool.W)))
            return hipErrorInvalidValue;
        if (r.pool.dx != nullptr && (r.pool.x == nullptr || r.pool.y == nullptr ||
                                     r.rows % ((int64_t)(r.pool.H / 2) * (r.pool.W / 2))))
            return hipErrorInvalidValue;
    }
    if (r.pool.dx_c32 != nullptr && (r.pool.dx == nullptr || r.out_p16 != nullptr || r.ldc % 32 != 0))
        return hipErrorInvalidValue;
    if (r.zero_cls != 0 && (r.out_p16 != nullptr || r.out_c4 != nullptr)) return hipErrorInvalidValue;
    if (r.pool3.out != nullptr) {
        const Pool3& p = r.pool3;
        if (r.out_p16 != nullptr || r.out_c4 != nullptr || r.zero_cls != 0 || r.pool.pool_out != nullptr ||
            r.pool.dx != nullptr || r.relu_mask != nullptr || p.arg == nullptr || r.ldc % 4 != 0 || p.H <= 0 ||
            p.W <= 0 || p.OH != (p.H - 1) / 2 + 1 || p.OW != (p.W - 1) / 2 + 1 || r.rows % ((int64_t)p.H * p.W) != 0)
            return hipErrorInvalidValue;
        Rq3Geom g;
        g.qpr = r.ldc / 4;
        g.H = p.H;
        g.W = p.W;
        g.OH = p.OH;
        static const int rows_env = getenv("NITI_RQ3_ROWS") ? atoi(getenv("NITI_RQ3_ROWS")) : RQ3_ROWS;
        static const int remap_env = getenv("NITI_RQ3_REMAP") ? atoi(getenv("NITI_RQ3_REMAP")) : 0;
        g.rows = rows_env > 0 ? rows_env : RQ3_ROWS;
        const int strips = (p.OH + g.rows - 1) / g.rows;
        const int64_t units = r.rows / ((int64_t)p.H * p.W) * strips * p.OW * g.qpr;
        if (units >= (int64_t)1 << 31) return hipErrorInvalidValue;
        g.units = (uint32_t)units;
        g.fq = make_fastdiv((uint32_t)g.qpr);
        g.fow = make_fastdiv((uint32_t)p.OW);
        g.fch = make_fastdiv((uint32_t)strips);
        int64_t blocks = (units + 255) / 256;
        g.remap = remap_env != 0 && blocks <= ((int64_t)1 << 24);
        if (!g.remap && blocks > 8192) blocks = 8192;
        if (blocks < 1) blocks = 1;
        if (r.relu)
            hipLaunchKernelGGL(requant_pool3_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, r, g);
        else
            hipLaunchKernelGGL(requant_pool3_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, r, g);
        return hipGetLastError();
    }
    if (r.out_p16 != nullptr) {  // the output (dx with the pool gradient) also as its P16 copy
        if (!requant_p16_ok(r)) return hipErrorInvalidValue;
        RqGeom g{};
        g.qpr = r.ldc / 4;
        g.W = r.pool.W;
        const int gsz = r.pool.dx == nullptr ? 16 : (r.pool.W == 16 ? p16_group<16>() : p16_group<8>());
        // plain: a thread per (16-row block, quad, quarter); pool gradient: per (run, quad)
        const int64_t units = r.rows / gsz * g.qpr * (r.pool.dx == nullptr ? 4 : 1);
        if (units >= (int64_t)1 << 31) return hipErrorInvalidValue;
        if (units == 0) return hipSuccess;
        g.units = (uint32_t)units;
        g.fq = make_fastdiv((uint32_t)g.qpr);
        int64_t blocks = (units + 255) / 256;
        if (blocks > 2048) blocks = 2048;
        if (r.pool.dx == nullptr)
            hipLaunchKernelGGL(requant_p16_plain_kernel, dim3((unsigned)blocks), dim3(256), 0, st, r, g);
        else
            launch_requant_p16<RQ_POOL_BWD>(r, g, blocks, st);
        return hipGetLastError();
    }
    if (r.out_c4 == nullptr) {
        const bool pf = r.pool.pool_out != nullptr, pb = r.pool.dx != nullptr;
        if (!pf && !pb && r.out_nhwc16 == nullptr) return hipErrorInvalidValue;
        RqGeom g;
        g.qpr = r.ldc / 4;
        g.W = r.pool.W;
        const int64_t rows = pf ? r.rows / 4 : r.rows;  // pooled pixels for the pool modes
        const int64_t units = rows * g.qpr;
        if (units >= (int64_t)1 << 31) return hipErrorInvalidValue;
        g.units = (uint32_t)units;
        g.fq = make_fastdiv((uint32_t)g.qpr);
        if (pf || pb) {
            g.fpw = make_fastdiv((uint32_t)(r.pool.W / 2));
            g.fph = make_fastdiv((uint32_t)(r.pool.H / 2));
        }
        if (r.zero_cls != 0) {
            if (pf || pb || r.zc_h <= 0 || r.zc_w <= 0 || r.rows % ((int64_t)r.zc_h * r.zc_w)) return hipErrorInvalidValue;
            g.fzw = make_fastdiv((uint32_t)r.zc_w);
            g.fzh = make_fastdiv((uint32_t)r.zc_h);
        }
        int64_t blocks = (units + 256 * RQ_U - 1) / (256 * RQ_U);
        if (blocks > 2048) blocks = 2048;
        if (blocks < 1) blocks = 1;
        if (pf)
            hipLaunchKernelGGL(requant_quad_kernel<RQ_POOL_FWD>, dim3((unsigned)blocks), dim3(256), 0, st, r, g);
        else if (pb)
            hipLaunchKernelGGL(requant_quad_kernel<RQ_POOL_BWD>, dim3((unsigned)blocks), dim3(256), 0, st, r, g);
        else
            hipLaunchKernelGGL(requant_quad_kernel<RQ_PLAIN>, dim3((unsigned)blocks), dim3(256), 0, st, r, g);
        return hipGetLastError();
    }
    const int64_t total = r.rows * (r.ldc / 16);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(requant_act_kernel, dim3((unsigned)blocks), dim3(256), 0, st, r);
    return hipGetLastError();
}

__global__ void requant_grad_kernel(const int32_t* __restrict__ acc, int64_t n, const uint32_t* __restrict__ amax,
                                    int rule, int8_t* __restrict__ g_out, int8_t* __restrict__ w) {
    const int bw = bitwidth_of(read_max(amax));
    const int s = bw - rule;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t g = bw == 0 ? 0 : psto_any(acc[i], s);
        if (g_out) g_out[i] = (int8_t)g;
        if (w) w[i] = (int8_t)clip127((int32_t)w[i] - g);
    }
}

hipError_t requant_grad(const int32_t* acc, int64_t n, const uint32_t* amax, int rule, int8_t* g_out, int8_t* w,
                        hipStream_t st) {
    if (n <= 0) return hipSuccess;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(requant_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, st, acc, n, amax, rule, g_out, w);
    return hipGetLastError();
}

}  // namespace niti
