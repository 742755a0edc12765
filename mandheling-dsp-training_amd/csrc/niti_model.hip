// niti_model.hip -- device-resident NITI int8 training step (+ RCCL data parallelism).
//
// One NITI_SGD step of the reference's NITIInt8Train (execution-engine/tools/train/source/
// demo/MnistUtils.cpp:68-147, optimizer/NITI_SGD.hpp:20-54) executed entirely on the GPU:
//   forward   : per layer NITI_Conv_Int8 (+ NITI_Relu_Int8, NITI_Maxpool_Int8)
//   loss      : NITI_LOSS_Grad_Int8 (NITI_CPULossGrad_Int8.cpp:81-200)
//   backward  : grad/NITI_Conv_Int8_Grad.cpp -- NITI_GradientCONV_Int8 (weight gradient) and
//               NITI_DeCONV_Int8 (input gradient, skipped for the first layer exactly as the
//               lazy reference graph skips it), pool / relu gradients
//   update    : w <- clip(w - g, +-127)  (NITI_SGD.hpp:49-52)
// With a communicator (exact mode) the input quantiser's statistics are all-reduced (SUM,
// MAX), every forward / input-gradient range with MAX and every int32 weight-gradient
// accumulator with SUM before it is requantised, so N ranks of batch b reproduce one device of
// batch N*b bit for bit.
// The network is a layer list (niti_chain_layer): LeNet, VGG-11 and VGG-16 are build()'s own tables,
// niti_model_create_chain brings the caller's, checked by chain_check before anything is allocated.
// What this driver shares with the ResNet-18 one (niti_resnet_model.hip) is its base, StepDriver
// (niti_step_driver.hpp): a Layer is the base's ParamLayer plus this driver's buffers, and the host
// access over the layers (weights and their derived copies, taps, logits, layer_info, spec_stats), the
// update jobs (sgd_job) and the GEMM weight gradient live there, over StepDriver::P.  Here: build(), the
// step with its capture, the per-layer phases, autotune, plans, get_input, and get_tap's choice of
// source.  The C ABI over both is niti_model_capi.hip.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <memory>
#include <vector>

#include "../../include/niti_hip.h"
#include "niti_map.hpp"
#include "niti_step_driver.hpp"

namespace niti {

namespace {
extern int g_p16_jobs_cap;
extern int g_wgrad_batch;
extern int g_wgrad_quad;
extern int g_c0w_mode;
extern unsigned long long g_c0w_launches;
}
void model_p16_jobs_cap(int cap) { g_p16_jobs_cap = cap <= 0 ? P16_MAX_JOBS : cap; }
void model_wgrad_batch(int mode) { g_wgrad_batch = mode < 0 ? 1 : mode; }
void model_wgrad_quad(int kg) { g_wgrad_quad = kg < 0 ? -1 : kg; }
int wgrad_quad_kg(int own) { return g_wgrad_quad >= 0 ? g_wgrad_quad : own; }
void model_conv0_wgrad_codes(int mode) { g_c0w_mode = mode < 0 ? -1 : (mode > 0 ? 1 : 0); }
unsigned long long model_conv0_wgrad_codes_launches() { return g_c0w_launches; }

namespace {

// im2col of the first layer: xcol[p][(ky * KW + kx) * C + c] = x[n][oy * sh + ky - pt][ox * sw + kx - pl][c]
// (NHWC16 input, zero outside the image and for k >= C * KH * KW), one output pixel (32 bytes) per
// thread; C / KH / KW as template arguments keep the byte positions compile-time (VGG 3/3/3,
// LeNet 1/5/5), 0 selects the runtime fallback.
template <int C, int KH, int KW>
struct Im2Col32 {
    const int8_t* x;
    int cip, h, w, oh, ow, c, kh, kw, sh, sw, pt, pl;
    int8_t* out;
    __device__ void operator()(int64_t p) const {
        typedef signed char v16c_t __attribute__((ext_vector_type(16)));
        const int64_t img = p / ((int64_t)oh * ow);
        const int r = (int)(p - img * oh * ow);
        const int oy = r / ow, ox = r - (r / ow) * ow;
        const int8_t* base = x + img * h * w * cip;
        if constexpr (C > 0) {
            v16c_t v[2] = {v16c_t{}, v16c_t{}};
#pragma unroll
            for (int ky = 0; ky < KH; ++ky)
#pragma unroll
                for (int kx = 0; kx < KW; ++kx) {
                    const int iy = oy * sh + ky - pt, ix = ox * sw + kx - pl;
                    const bool ok = iy >= 0 && iy < h && ix >= 0 && ix < w;
                    // the pixel's first 16 channels in one 16-byte load (zeros outside the image)
                    const v16c_t px = ok ? *(const v16c_t*)(base + ((int64_t)iy * w + ix) * cip) : v16c_t{};
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) {
                        const int k = (ky * KW + kx) * C + ch;
                        v[k >> 4][k & 15] = px[ch];
                    }
                }
            *(v16c_t*)(out + p * 32) = v[0];
            *(v16c_t*)(out + p * 32 + 16) = v[1];
        } else {
            int k = 0;
            for (int ky = 0; ky < kh; ++ky)
                for (int kx = 0; kx < kw; ++kx) {
                    const int iy = oy * sh + ky - pt, ix = ox * sw + kx - pl;
                    const bool ok = iy >= 0 && iy < h && ix >= 0 && ix < w;
                    for (int ch = 0; ch < c; ++ch, ++k)
                        out[p * 32 + k] = ok ? base[((int64_t)iy * w + ix) * cip + ch] : (int8_t)0;
                }
            for (; k < 32; ++k) out[p * 32 + k] = 0;
        }
    }
};

// diagnostic: jobs per P16 conversion launch (niti_diag_p16_jobs_cap)
int g_p16_jobs_cap = P16_MAX_JOBS;
// the step's P16 weight gradients as one launch (niti_diag_wgrad_batch): 0 off, 1 the model's own
// item size (WGRAD_BATCH_T until autotuned, which may turn it off), >= 2 that item size;
// NITI_WGRAD_BATCH sets the process's starting mode
int g_wgrad_batch = getenv("NITI_WGRAD_BATCH") != nullptr ? std::max(0, atoi(getenv("NITI_WGRAD_BATCH"))) : 1;
constexpr int WGRAD_BATCH_T = 256;
// the batch's quad threshold (niti_diag_wgrad_quad): -1 the schedule owner's own (the model's
// wgb_quad, the op entry's P16_QUAD_KG), 0 no quad items, k > 0 that many K groups; NITI_WGRAD_QUAD
// sets the process's starting value
int g_wgrad_quad = getenv("NITI_WGRAD_QUAD") != nullptr ? std::max(-1, atoi(getenv("NITI_WGRAD_QUAD"))) : -1;
// the first layer's weight gradient from the pooled gradient and the pool codes
// (niti_diag_conv0_wgrad_codes): -1 the model's choice, 0 off, 1 on where eligible;
// NITI_CONV0_WGRAD_CODES sets the process's starting value.  g_c0w_launches counts the step's launches.
int g_c0w_mode = getenv("NITI_CONV0_WGRAD_CODES") != nullptr
                     ? std::min(1, std::max(-1, atoi(getenv("NITI_CONV0_WGRAD_CODES"))))
                     : -1;
unsigned long long g_c0w_launches = 0;

static hipError_t im2col32(const ConvGeom& o, const int8_t* x16, int8_t* out, hipStream_t st) {
    const int64_t px = (int64_t)o.n * o.oh * o.ow;
    const int cip = round_up(o.c_in, 16);
    if (o.c_in == 3 && o.kh == 3 && o.kw == 3)
        return launch_map(px, Im2Col32<3, 3, 3>{x16, cip, o.h, o.w, o.oh, o.ow, 3, 3, 3, o.sh, o.sw, o.pt, o.pl, out}, st);
    if (o.c_in == 1 && o.kh == 5 && o.kw == 5)
        return launch_map(px, Im2Col32<1, 5, 5>{x16, cip, o.h, o.w, o.oh, o.ow, 1, 5, 5, o.sh, o.sw, o.pt, o.pl, out}, st);
    return launch_map(px, Im2Col32<0, 0, 0>{x16, cip, o.h, o.w, o.oh, o.ow, o.c_in, o.kh, o.kw, o.sh, o.sw, o.pt, o.pl,
                                            out},
                      st);
}

// NCHW flatten of a pooled NHWC16 map: out[n][c*HW + p] = in[n][p][c] (c < C); LeNet's
// _Reshape(x, {0, -1, 1, 1}) after _Convert(x, NCHW) (mnistTrain.cpp:175-176).
struct FlattenFwd {
    const int8_t* in;
    int hw, c, cp, ldo;
    int8_t* out;
    __device__ void operator()(int64_t i) const {  // i over [n][ldo]
        const int64_t b = i / ldo;
        const int j = (int)(i - b * ldo);
        const int ch = j / hw, p = j - ch * hw;
        out[i] = ch < c ? in[(b * hw + p) * cp + ch] : (int8_t)0;
    }
};
struct FlattenBwd {
    const int8_t* dout;
    int hw, c, cp, ldo;
    int8_t* din;
    __device__ void operator()(int64_t i) const {  // i over [n][hw][cp]
        const int ch = (int)(i % cp);
        const int64_t r = i / cp;
        const int p = (int)(r % hw);
        const int64_t b = r / hw;
        din[i] = ch < c ? dout[b * ldo + ch * hw + p] : (int8_t)0;
    }
};

// The expanded output gradient of a 2x2-pooled layer from its pooled gradient and the recorded route:
// out[n][y][x][c] = g0[n][y / 2][x / 2][c] where bit 2 (y & 1) + (x & 1) of the code is set, else 0
// (the first layer's dy tap after a step on the codes route, which never writes that tensor).
struct ExpandPoolCodes {
    const int8_t* g0;
    const int8_t* code;
    int oh, ow, cop;
    int8_t* out;
    __device__ void operator()(int64_t i) const {  // i over [n][oh][ow][cop]
        const int c = (int)(i % cop);
        int64_t r = i / cop;
        const int x = (int)(r % ow);
        r /= ow;
        const int y = (int)(r % oh);
        const int64_t b = r / oh;
        const int64_t q = ((b * (oh / 2) + (y >> 1)) * (ow / 2) + (x >> 1)) * cop + c;
        out[i] = ((code[q] >> (2 * (y & 1) + (x & 1))) & 1) ? g0[q] : (int8_t)0;
    }
};

}  // namespace

// one layer of the chain: the parameter layer the base knows (ParamLayer: geometry, weights and their
// derived copies, the weight gradient) and this driver's activation / gradient buffers and routes
struct Layer : ParamLayer {
    int flatten = 0;
    // a global sum pool after the relu (niti_chain_layer3): r [n][oh][ow][cop] summed per image and channel
    // into gsum (sum_pool_wide, its range in gp_amax), requantised into flat [n][cop] with exponent exp_gp;
    // the next layer's input gradient lands in dflat and sum_pool_grad hands it to every pixel of dy
    int gpool = 0;
    int32_t* gsum = nullptr;
    int8_t* exp_gp = nullptr;
    uint32_t* gp_amax = nullptr;
    // a residual sum after the conv (niti_chain_layer3): skip = d > 0 adds the final output of layer i - d
    // (its r, exponent exp) to this layer's requantised conv output (the model's sum_tmp, exponent ey), and
    // the requantised sum (+ relu) is r; src_of = j >= 0 on the source names that adding layer, whose
    // output gradient joins layer i + 1's unmasked input gradient (sum_tmp, exponent the model's e_tmp) in
    // this layer's dy.  sum_amax: the range of the forward sum (adding layer) / the gradient sum (source).
    // Neither kind runs on the row kernels or as the head: every tensor the sums read is NHWC16.
    int skip = 0, src_of = -1;
    int8_t* ey = nullptr;
    uint32_t* sum_amax = nullptr;   // (adding layer)
    uint32_t* bsum_amax = nullptr;  // (source)
    int8_t* edy = nullptr;  // the exponent of dy (kept where the model has a skip: has_skip)
    int ph = 0, pw = 0;      // pooled size
    int8_t* r = nullptr;     // conv (+relu) output NHWC16 [n][oh][ow][cop]
    int8_t* p = nullptr;     // pooled NHWC16
    // the 2x2 pool's gradient route recorded by the forward (pool_code4, [n][ph][pw][cop] bytes; the
    // pooled layers whose forward and next input gradient run on the kernels that know it)
    int8_t* pc = nullptr;
    bool r_written = false;  // this step wrote r (a pooled layer with a recorded route skips it
                             // under keep_grads(0): nothing else reads it; its tap is then invalid)
    int8_t* flat = nullptr;  // flattened NHWC16 [n][1][1][c*ph*pw]
    int8_t* dy = nullptr;    // output gradient NHWC16 [n][oh][ow][cop]
    int8_t* dtmp = nullptr;  // gradient wrt the pooled / flattened output
    int8_t* dflat = nullptr;
    // the P16 weight gradient's own split-K slabs when its combine is deferred to the NITI_SGD
    // launch (sgd_update_many); the deferred combine itself is ParamLayer::defer, as the GEMM path's
    int32_t* slab16 = nullptr;
    size_t slab16_bytes = 0;
    bool fc_sgd = false;  // this step's weight gradient took the fused NITI_SGD form (pass 1 in run())
    int8_t* exp = nullptr;   // exponent of this layer's output
    const int8_t* oexp() const { return gpool ? exp_gp : exp; }  // ... of what the next layer reads
    bool to_1x1() const { return flatten || gpool; }             // the next layer reads flat, a 1x1 map
    const int8_t* in = nullptr;  // NHWC16 input (previous output or x0)
    // First layer with C_in * KH * KW <= 32 (VGG: 3 x 3 x 3, LeNet: 1 x 5 x 5): the conv runs as a
    // 1x1 conv over an im2col copy of its input (xcol [pixels][32], k = (ky * KW + kx) * C_in + c,
    // zero padded), so its GEMMs take K = 32 instead of 16 channels x 9 taps and the padded taps
    // cost nothing.  g is that 1x1 geometry and kp = 32 marks the layer; og the layer as the network
    // defines it (reported, weights and taps converted to / from it on the host).
    int8_t* xcol = nullptr;
    // stride-1 pad-1 3x3 layers on the register-fed forward with the fused rescale (rc;
    // niti_rowconv.hip): its C32 input copy, the grid-barrier epoch
    int8_t* xc32 = nullptr;
    uint32_t epoch = 0;
    // its input gradient on the same kernel (rcd: rotated transposed weights in wft, dy in C32, the
    // previous layer's relu / pool gradient in the epilogue); dg = that conv's geometry
    ConvGeom dg{};
    int8_t* dyc32 = nullptr;
    // what a flatten reads and its gradient writes: the pooled map, or the conv (+relu) output itself
    int fh() const { return pool ? ph : g.oh; }
    int fw() const { return pool ? pw : g.ow; }
    const int8_t* fsrc() const { return pool ? p : r; }
};

struct Model final : StepDriver {
    int arch = 0, in_c = 0, in_h = 0, in_w = 0;
    std::vector<Layer> L;
    int8_t* x0 = nullptr;   // NHWC16 input
    int8_t* exp0 = nullptr; // input exponent
    int32_t* acc = nullptr; // shared fwd / dgrad accumulator
    // P16 copies of the weight-gradient operands (niti_wgrad.hip): one input copy per layer (all
    // converted together when the backward pass starts, off the step stream) and one
    // output-gradient copy per layer, written by the input-gradient requantisation that produces
    // dy (requant_act's out_p16) where that pass can, else converted before the weight gradient
    int32_t* grad_bucket = nullptr;  // every layer's dwacc, contiguous
    // the step's update jobs, one per layer, and the ones the batched update takes (sized in build_chain:
    // nothing is allocated inside a step); more than SGD_MAX_JOBS of them go in consecutive launches
    std::vector<SgdJob> sgd_jobs, sgd_many;
    // a list with a residual sum: every output gradient carries its exponent on the device (Layer::edy; the
    // loss gradient's is 0), the conv output / input gradient ahead of a sum waits in sum_tmp
    bool has_skip = false;
    int8_t* sum_tmp = nullptr;
    int8_t* e_tmp = nullptr;
    int skip_sum_fwd(int i, hipStream_t st);
    int skip_sum_bwd(int s, hipStream_t st);
    size_t grad_bucket_elems = 0;
    std::vector<int8_t*> xp16, dp16;
    std::vector<char> dp16_valid;  // dp16[i] holds L[i].dy as it is now
    std::vector<char> xp16_valid;  // xp16[i] holds L[i].in as it is now (cleared when a step starts)
    void invalidate_xp16() { std::fill(xp16_valid.begin(), xp16_valid.end(), 0); }
    bool fuse_dp16 = true;    // dy's P16 copy written by the requantisation that produces dy
    // register-fed forward (niti_rowconv.hip) for the layers it takes; xc32_valid[i]: L[i].xc32
    // holds L[i].in as it is now (written by the previous layer's epilogue, else converted)
    std::vector<char> xc32_valid;
    // a fully connected layer's weight gradient as a range pass plus a recompute that applies
    // NITI_SGD in its epilogue (conv_wgrad_fc_sgd): single device, inside run() (NITI_FC_SGD=0: off)
    bool fc_sgd_layer(int i) const {
        static const bool off = getenv("NITI_FC_SGD") && atoi(getenv("NITI_FC_SGD")) == 0;
        const ConvGeom& g = L[i].g;
        return in_step && !off && !dp() && !tuning && !L[i].dw && conv_wgrad_fc_sgd_ok(g) &&
               !(head_layer(i) && g.c_out <= 32 && g.cip % 32 == 0) && wgrad_p16_splits(i) == 0;
    }
    // the GEMM speculative pairs' alternates (one bit width below / above A's guess), shared by every
    // layer phase: a pair's B consumes them before the next pair's A writes them
    int8_t* gspec_alt = nullptr;
    size_t gspec_alt_bytes = 0;
    // the first layer's range came with its im2col copy (input_im2col's Conv0Range) this step
    bool conv0_ranged = false;
    // the first layer's im2col copy comes straight from the batch (input_im2col).  That kernel stages
    // rows of w + kw - 1 pixels, which hold every tap only while 2 pad < kernel; a wider pad goes
    // through x0 and im2col32, which bounds-checks each tap.
    static bool input_fused_ok(int c_in, int k, int pad) { return input_im2col_ok(c_in, k, k) && 2 * pad < k; }
    static bool input_fused(const Layer& f) {
        const ConvGeom& o = f.og;
        return f.kp && o.kh == o.kw && o.pt == o.pl && input_fused_ok(o.c_in, o.kh, o.pt) && o.sh == 1 && o.sw == 1;
    }
    bool rowconv_layer(int i) const { return use_rowconv && L[i].rc; }
    // dyc32_valid[i]: L[i].dyc32 holds L[i].dy as it is now (written by the next layer's input
    // gradient epilogue, else converted)
    std::vector<char> dyc32_valid;
    // dy16_valid[i]: L[i].dy (NHWC16) was written this step; a row-kernel input gradient leaves it
    // out when the layer's own consumers read its C32 (input gradient) and P16 (weight gradient)
    // copies (niti_model_get_tap rebuilds it from the C32 copy)
    std::vector<char> dy16_valid;
    bool rowconv_dgrad_layer(int i) const { return use_rowconv && L[i].rcd; }
    // layer i's 2x2 pool route travels as codes (Layer::pc): its forward (the first layer's conv0
    // kernel or a row kernel) records it and layer i + 1's input gradient (a row kernel, or the
    // head's) reads it instead of the pre-pool output and the pooled one
    bool pool_code_layer(int i) const {
        const Layer& l = L[i];
        if (!l.pool || l.flatten || l.pc == nullptr || i + 1 >= (int)L.size()) return false;
        const bool fwd = (l.kp && conv0_ok(l.g)) || rowconv_layer(i);
        const bool bwd = rowconv_dgrad_layer(i + 1) || head_dgrad_ok(i + 1);
        return fwd && bwd;
    }
    // the classifier head (a 1x1 conv over 1x1 maps, at most 64 outputs) on the row kernel's
    // W = 1 path: forward, and its input gradient into the previous layer's relu / 2x2 pool
    bool head_layer(int i) const {
        const Layer& l = L[i];
        const ConvGeom& g = l.g;
        return use_rowconv && !l.kp && l.bar != nullptr && g.kh == 1 && g.kw == 1 && g.h == 1 && g.w == 1 &&
               g.c_out <= 64 && !l.pool && !l.flatten && !l.skip && l.src_of < 0;
    }
    bool head_dgrad_ok(int i) const {
        if (i == 0 || !head_layer(i)) return false;
        const Layer& pv = L[i - 1];
        if (pv.to_1x1() || pv.kp || pv.src_of >= 0 || pv.g.cop != L[i].g.cip) return false;
        return pv.pool ? (pv.ph == 1 && pv.pw == 1 && pv.g.oh == 2 && pv.g.ow == 2) : (pv.g.oh == 1 && pv.g.ow == 1);
    }
    // The first layer's expanded output gradient has one reader, its own weight gradient (no input
    // gradient; no tap under keep_grads(0)).  On this route layer 1's input gradient writes only the
    // pooled gradient g0 -- the plain `out` epilogue, into the first quarter of L[0].dy -- and the
    // weight gradient reads g0, the codes and xcol (conv0_wgrad_codes).  Single device, outside a
    // graph capture (its combine is deferred to the update launch; a captured step keeps the old
    // launches) and without the side stream, layer 1's input gradient a W > 0 row launch, no probe on
    // the launch it replaces.
    int32_t* c0w_slab = nullptr;  // the route's own slabs
    size_t c0w_slab_bytes = 0;
    bool c0w_tuned = true;   // the model's choice (mode -1): the autotuner's, else the default
    int c0w_force = -1;      // the autotuner's own timing: 0 / 1 that way, whatever the mode
    bool dy0_codes = false;  // the last step left g0 in L[0].dy, not the expanded gradient (get_tap rebuilds it)
    bool conv0_codes_eligible() const {
        if (L.size() < 2 || c0w_slab == nullptr) return false;
        const Layer& l = L[0];
        if (!l.kp || !pool_code_layer(0) || keep_grads || coll != nullptr || coll_grad != nullptr) return false;
        if (l.og.sh != 1 || l.og.sw != 1) return false;  // (measured and tested on stride-1 first layers only)
        if (use_graph || capturing || overlap) return false;  // (one stream, direct launches: the bench's step)
        if (!rowconv_dgrad_layer(1) || rowconv_seg(L[1].dg) || head_dgrad_ok(1)) return false;
        if (probe_layer == 0 && probe_phase == 2) return false;
        return conv0_wgrad_codes_ok(l.g.n, l.g.oh, l.g.ow, l.g.cop, l.g.cip);
    }
    bool conv0_codes_route() const {
        if (c0w_force >= 0) return c0w_force == 1 && conv0_codes_eligible();
        if (tuning || g_c0w_mode == 0 || (g_c0w_mode < 0 && !c0w_tuned)) return false;
        return conv0_codes_eligible();
    }
    int tune_conv0_codes(hipStream_t st, TuneTimer& timer, bool log);
    // jobs per P16 conversion launch: P16_MAX_JOBS, lowered only by niti_diag_p16_jobs_cap (tests
    // reach the more-than-one-launch branches with a small net)
    static int p16_jobs_cap() { return std::min(std::max(g_p16_jobs_cap, 1), P16_MAX_JOBS); }
    // every P16 input copy of the backward pass as one job list (false: more than one launch holds)
    bool p16_input_jobs(P16Conv* jobs, int* n) {
        *n = 0;
        for (int j = 0; j < (int)L.size(); ++j)
            if (wgrad_p16_splits(j)) {
                if (*n == p16_jobs_cap()) return false;
                const ConvGeom& g = L[j].g;
                jobs[(*n)++] = P16Conv{L[j].in, (int64_t)g.n * g.h * g.w, g.cip, xp16[j]};
            }
        return true;
    }
    int convert_p16_inputs(hipStream_t st) {
        P16Conv jobs[P16_MAX_JOBS];
        int n = 0;
        for (int j = 0; j < (int)L.size(); ++j)
            if (wgrad_p16_splits(j)) {
                const ConvGeom& g = L[j].g;
                jobs[n++] = P16Conv{L[j].in, (int64_t)g.n * g.h * g.w, g.cip, xp16[j]};
                xp16_valid[j] = 1;
                if (n == p16_jobs_cap() || j + 1 == (int)L.size()) {
                    if (nhwc16_to_p16_many(jobs, n, st) != hipSuccess) return NITI_NO_EXECUTION;
                    n = 0;
                }
            }
        if (n > 0 && nhwc16_to_p16_many(jobs, n, st) != hipSuccess) return NITI_NO_EXECUTION;
        return NITI_NO_ERROR;
    }
    // the K split the P16 weight gradient of layer i runs with, 0 when layer i runs on the NHWC16
    // kernels (a plan override of another tile, or a geometry the P16 kernel does not take)
    int wgrad_p16_splits(int i) const {
        const ConvGeom& g = L[i].g;
        if (L[i].dw || !conv_wgrad_p16_ok(g)) return 0;
        PlanChoice c;
        if (plan_override_lookup(conv_plan_key(PLAN_WGRAD, g), &c)) return c.bm == PLAN_P16_TILE ? c.splits : 0;
        return conv_wgrad_p16_splits(g);
    }
    // the probed launch's own begin / end events and span slot (P16 weight gradient)
    void probe_launch(int layer, int phase, hipEvent_t* b, hipEvent_t* e, unsigned long long** sp) {
        *b = *e = nullptr;
        *sp = nullptr;
        if (!probe_armed(layer, phase)) return;
        if (probe_count < (int)ev0.size()) {
            *b = ev0[probe_count];
            *e = ev1[probe_count];
            ++probe_count;
        }
        if (span != nullptr && span_count < span_cap) *sp = span + 2 * SPAN_MAX_BLOCKS * span_count++;
    }
    // The weight gradient of layer i and the input gradient of layer i both read dy_i and
    // nothing else the other writes, so the weight gradients run on a second stream, each
    // released by an event after its dy is produced, and overlap the input-gradient chain
    // (the launches are small enough that one alone leaves most of the chip idle).  The SGD
    // launch joins the two streams.
    bool overlap = true;
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> ev_dy;
    hipEvent_t ev_side = nullptr;
    uint32_t* amax = nullptr;  // 3 ranges per layer (forward, input gradient, weight gradient)
    size_t amax_bytes = 0;
    uint32_t* rng(int layer, int which) { return amax + (size_t)(3 * layer + which) * MAX_WORDS; }
    // input quantiser statistics {S1, S2, xmax, 255 - xmin} (niti_quant.hip)
    unsigned long long* qstats = nullptr;
    unsigned long long* qslots = nullptr;  // per-block partial statistics (IMAGE_STATS_SLOTS x 4)
    int8_t* x0n = nullptr;                 // the int8 input NCHW (written by the fused input pass)
    bool x0_nchw_valid = false;
    // Optional hipGraph replay of the single-device step: ~95 launches become one graph launch
    // (or three when a probe splits it around the probed GEMM).  Captured on an internal
    // stream, fenced against the caller's stream with events; re-captured when the captured
    // inputs (input / label pointers, input exponent, probe target) change.  Off by default:
    // on ROCm 7.2 the replayed step measured 0.97 ms against 0.84 ms for direct launches (each
    // graph kernel node ran slower, e.g. the probed GEMM + reduce 43 us vs 33 us).
    std::vector<hipGraphExec_t> segs;
    struct Key {
        const void* x = nullptr;
        const void* labels = nullptr;
        int exp_in = 0, pl = -1, pp = -1;
        bool operator==(const Key& o) const {
            return x == o.x && labels == o.labels && exp_in == o.exp_in && pl == o.pl && pp == o.pp;
        }
    } key;
    hipError_t cap_err = hipSuccess;
    void drop_graph() override {
        for (auto e : segs) (void)hipGraphExecDestroy(e);
        segs.clear();
    }
    // close the current capture into a segment and open the next one
    void seg_cut(hipStream_t st) {
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamEndCapture(st, &g);
        hipGraphExec_t ex = nullptr;
        if (e == hipSuccess) e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
        if (g) (void)hipGraphDestroy(g);
        if (e == hipSuccess) segs.push_back(ex);
        if (cap_err == hipSuccess) cap_err = e;
        e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
        if (cap_err == hipSuccess) cap_err = e;
    }
    // kernel probe: HIP events around one GEMM (layer, phase 0 fwd / 1 dgrad / 2 wgrad); in a
    // graph the probe points are segment boundaries and the events go between the launches
    // kernel-span probe (weight gradient): per launch {min block start, max block end} on the
    // device wall clock, written by the kernel itself (niti_kernels.hpp probe_span_arm)
    unsigned long long* span = nullptr;
    int span_cap = 0, span_count = 0;
    void arm_kernel_events(int layer, int phase) {
        if (!probe_armed(layer, phase) || probe_count >= (int)ev0.size()) return;
        probe_events_arm(ev0[probe_count], ev1[probe_count]);
        ++probe_count;
    }
    void arm_span(int layer, int phase) {
        if (!probe_armed(layer, phase) || span == nullptr || span_count >= span_cap) return;
        probe_span_arm(span + 2 * SPAN_MAX_BLOCKS * span_count++);
    }
    void probe(int layer, int phase, bool begin, hipStream_t st) {
        if (layer != probe_layer || phase != probe_phase || tuning) return;
        if (capturing) {
            seg_cut(st);
            return;
        }
        if (probe_paused) return;
        if (probe_count >= (int)ev0.size()) return;
        if (begin) {
            (void)hipEventRecord(ev0[probe_count], st);
        } else {
            (void)hipEventRecord(ev1[probe_count], st);
            ++probe_count;
        }
    }
    // the end event of a probe that the callee records itself (right after the GEMM launch)
    hipEvent_t probe_end_event(int layer, int phase) {
        if (!probe_armed(layer, phase) || probe_count >= (int)ev0.size()) return nullptr;
        return ev1[probe_count++];
    }
    void clear_probe() override {
        StepDriver::clear_probe();
        if (span) (void)hipFree(span);
        span = nullptr;
        span_cap = span_count = 0;
    }
    int probe_alloc(int phase, int max_launches) override;
    int probe_read_span(double* total_ms, int* count) override;

    int build(int arch_, int batch_, int in_hw = 0);
    // the model of a layer list (c_in and the map sizes derived as chain_check derives them); the
    // built-in networks are build()'s own lists
    int build_chain(int arch_, int batch_, const niti_chain_layer3* layers, int n, int in_c_, int in_hw, int rule);
    int layer_skip(int layer, int* skip, int* gpool) const override {
        if (!layer_ok(layer)) return NITI_INVALID_VALUE;
        *skip = L[layer].skip;
        *gpool = L[layer].gpool;
        return NITI_NO_ERROR;
    }
    // the conv (+ relu, pool, flatten) of layer i's forward; fwd_layer adds the global pool
    int fwd_conv_layer(int i, hipStream_t st);
    int gpool_fwd(int i, hipStream_t st);
    int fwd_layer(int i, hipStream_t st);
    int wgrad_layer(int i, hipStream_t st);
    int dgrad_layer(int i, hipStream_t st);
    // the input gradient of layer i need not write L[i - 1].dy in NHWC16: its weight gradient reads
    // the P16 copy (p16) and its input gradient the C32 copy (next) this same launch writes (layer 0's
    // GEMM weight gradient reads NHWC16).  NITI_DY16=1 keeps the copy (A/B diagnostics).
    // the classifier head's whole chain (forward, loss gradient, weight and input gradient into the
    // previous layer's pool routes) as one launch (niti_head.hip): single device, the head on the
    // row kernel's W = 1 path after a pooled layer whose routes travel as codes (VGG-11)
    bool head_chain_on() const {
        const int h = (int)L.size() - 1;
        if (!head_chain_enabled() || h < 1 || dp() || tuning || probe_layer == h || has_skip) return false;
        const Layer& l = L[h];
        return head_layer(h) && head_dgrad_ok(h) && L[h - 1].pool && pool_code_layer(h - 1) &&
               head_chain_ok(batch, l.g.cip, l.g.c_out, l.g.cop) && L[h - 1].g.cop == l.g.cip && l.g.kh * l.g.kw == 1;
    }
    bool skip_dy16(int i, const int8_t* next, const int8_t* p16) const {
        static const bool keep = getenv("NITI_DY16") != nullptr && getenv("NITI_DY16")[0] == '1';
        return !keep && i - 1 >= 1 && next != nullptr && p16 != nullptr && wgrad_p16_splits(i - 1) > 0;
    }
    int autotune(hipStream_t st, int reps) override;
    int tune_wgrad_batch(hipStream_t st, TuneTimer& timer, bool log);
    size_t ws_bytes_for(int op) const { return op == PLAN_WGRAD ? slab_w_bytes : slab_bytes; }
    // The P16 weight gradients of a step as one persistent launch after the last input gradient
    // (conv_wgrad_p16_many): single device, one stream.  A weight gradient reads only its layer's
    // xp16 / dp16, which live until the backward pass ends, so every P16 layer but one with an armed
    // weight-gradient probe joins; the schedule and its device table are rebuilt outside the step
    // (and outside a capture) when a plan, the item size or the probe changes.
    int wgb_tuned = WGRAD_BATCH_T;  // the model's item size (K groups), 0: the autotuner turned the batch off
    int wgb_quad = P16_QUAD_KG;     // the model's quad threshold (K groups), 0: the autotuner turned quads off
    WgP16Many wgb;
    std::vector<int> wgb_layers;    // the layers of wgb's jobs, in job order (empty: no batch)
    void* wgb_dev = nullptr;
    size_t wgb_dev_bytes = 0;
    unsigned wgb_epoch = 0;
    int wgb_t = -1, wgb_q = -1, wgb_probe = -2;
    int wgrad_batch_t() const {
        if (dp() || g_wgrad_batch == 0) return 0;
        return g_wgrad_batch == 1 ? wgb_tuned : g_wgrad_batch;
    }
    int build_wgrad_batch(int t) { return build_wgrad_batch(t, wgrad_quad_kg(wgb_quad)); }
    int build_wgrad_batch(int t, int q) {
        const int pl = probe_phase == 2 ? probe_layer : -1;
        if (wgb_t == t && wgb_q == q && wgb_probe == pl && wgb_epoch == plan_override_epoch()) return NITI_NO_ERROR;
        drop_graph();  // (a captured step launched the old schedule)
        wgb.clear();
        wgb_layers.clear();
        wgb_t = t;
        wgb_q = q;
        wgb_probe = pl;
        wgb_epoch = plan_override_epoch();
        if (t <= 0) return NITI_NO_ERROR;
        WgP16Job jobs[P16_MANY_MAX_JOBS];
        std::vector<int> layers;
        for (int i = 0; i < (int)L.size(); ++i) {
            if (wgrad_p16_splits(i) <= 0 || i == pl) continue;
            if ((int)layers.size() == P16_MANY_MAX_JOBS) return NITI_NO_ERROR;  // (more than one launch holds: per layer)
            Layer& l = L[i];
            WgP16Job& j = jobs[layers.size()];
            j.g = l.g;
            j.x_p16 = xp16[i];
            j.dy_p16 = dp16[i];
            j.acc = l.dwacc;
            j.amax = rng(i, 2);
            j.slab = l.slab16;
            j.slab_bytes = l.slab16_bytes;
            layers.push_back(i);
        }
        if (layers.size() < 2) return NITI_NO_ERROR;
        int cus = 0, dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
            return NITI_NO_EXECUTION;
        if (conv_wgrad_p16_many_build(jobs, (int)layers.size(), cus, t, q, &wgb) != hipSuccess) return NITI_NO_EXECUTION;
        // (the previous table may still be read by a step in flight)
        if (hipDeviceSynchronize() != hipSuccess) return NITI_NO_EXECUTION;
        if (wgb.table_bytes > wgb_dev_bytes) {
            wgb_dev = ws.replace(wgb_dev, wgb.table_bytes);
            wgb_dev_bytes = wgb_dev ? wgb.table_bytes : 0;
            if (!wgb_dev) {
                wgb.clear();
                return NITI_OUT_OF_MEMORY;
            }
        }
        if (hipMemcpy(wgb_dev, wgb.table, wgb.table_bytes, hipMemcpyHostToDevice) != hipSuccess) {
            wgb.clear();
            return NITI_NO_EXECUTION;
        }
        wgb_layers = layers;
        return NITI_NO_ERROR;
    }
    bool wgrad_batched(int i) const {
        return std::find(wgb_layers.begin(), wgb_layers.end(), i) != wgb_layers.end();
    }
    // the batch launch and every member's combine fields (Layer::defer) or, where the combine is not
    // deferred to the update launch, its reduce
    int wgrad_batch_run(bool defer, hipStream_t st) {
        DTRY(conv_wgrad_p16_many(wgb, wgb_dev, st));
        for (size_t k = 0; k < wgb_layers.size(); ++k) {
            Layer& l = L[wgb_layers[k]];
            SgdJob& d = l.defer;
            d = SgdJob{};
            l.fc_sgd = false;
            if (wgb.splits[k] < 2) continue;
            const int64_t n = (int64_t)l.g.c_out * 9 * l.g.cip;
            if (defer) {
                d.slab = l.slab16;
                d.splits = wgb.splits[k];
                d.slab_stride = wgb.slab_stride[k];
                d.slab_n = n;
            } else {
                DTRY(splitk_reduce_linear(l.slab16, wgb.splits[k], n, wgb.slab_stride[k], l.dwacc,
                                          rng(wgb_layers[k], 2), st));
            }
        }
        return NITI_NO_ERROR;
    }
    int ensure_streams() {
        if (side) return NITI_NO_ERROR;
        if (hipStreamCreateWithFlags(&side, hipStreamNonBlocking) != hipSuccess) return NITI_NO_EXECUTION;
        // cross-stream hand-offs on one device need a device-scope release only (the default
        // system-scope fence writes back and invalidates the caches: ~7 us per record, measured)
        constexpr unsigned kFlags = hipEventDisableTiming | hipEventReleaseToDevice;
        if (hipEventCreateWithFlags(&ev_side, kFlags) != hipSuccess) return NITI_NO_EXECUTION;
        ev_dy.resize(L.size());
        for (auto& e : ev_dy)
            if (hipEventCreateWithFlags(&e, kFlags) != hipSuccess) return NITI_NO_EXECUTION;
        return NITI_NO_ERROR;
    }
    int run(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st);
    int step(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st) override;
    // the step's forward half: input (quantiser), every layer's forward -- all but the head's when
    // the head chain launch of run() does it (skip_head)
    int forward(const int8_t* x_nchw, int exp_in, const uint8_t* images, bool skip_head, hipStream_t st);
    int backward(bool head_chain, const int32_t* labels, SgdJob* jobs, hipStream_t st);
    int eval(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st) override;
    int copy_weights_from(StepDriver& src, hipStream_t st) override;
    int run_phase(int layer, int phase, hipStream_t st) override;
    int plan_info(int layer, int phase, int info[4]) override;
    int plan_set(int layer, int phase, const int plan[4]) override;
    void set_overlap(bool enable) override { overlap = enable; }
    // host access
    int get_tap(int layer, int which, int8_t* host, size_t bytes, hipStream_t st) override;
    void logits_view(const int8_t** logits, int* classes, int* ld, const int8_t** exp) const override {
        const Layer& t = L.back();
        *logits = t.r;
        *classes = t.g.c_out;
        *ld = t.g.cop;
        *exp = t.exp;
    }
    int get_input(int8_t* host, int* ascale, hipStream_t st) override;
    ~Model() override {  // (the rest, in order, in ~StepDriver)
        clear_probe();
        drop_graph();
        if (cst) (void)hipStreamSynchronize(cst);
        for (auto e : ev_dy) (void)hipEventDestroy(e);
        if (ev_side) (void)hipEventDestroy(ev_side);
        if (side) (void)hipStreamDestroy(side);
    }
};

static void add_conv(Model& m, int ci, int co, int k, int pad, int h, int relu, int pool, int flatten = 0, int dw = 0,
                     int stride = 1, int gpool = 0, int skip = 0) {
    Layer l;
    l.dw = dw;
    l.gpool = gpool;
    l.skip = skip;
    l.g.n = m.batch;
    l.g.c_in = ci;
    l.g.h = l.g.w = h;
    l.g.c_out = co;
    l.g.kh = l.g.kw = k;
    l.g.sh = l.g.sw = stride;
    l.g.pt = l.g.pl = l.g.pb = l.g.pr = pad;
    l.g.dh = l.g.dw = 1;
    l.g.finalize();
    l.og = l.g;
    // a strided 1x1 conv over a 1x1 map is the stride-1 layer: run as that (og keeps what the list says)
    if (stride != 1 && h == 1 && k == 1 && pad == 0) {
        l.g.sh = l.g.sw = 1;
        l.g.finalize();
    }
    l.relu = relu;
    l.pool = pool;
    l.flatten = flatten;
    if (pool) {
        l.ph = (l.g.oh - 2) / 2 + 1;
        l.pw = (l.g.ow - 2) / 2 + 1;
    }
    m.L.push_back(l);
}

// the largest tensor of a list's layer (elements, at the model's batch): the GEMM loaders address
// int8 operands with 31-bit byte offsets and the int32 accumulator of a tensor is four times its size
constexpr int64_t CHAIN_MAX_ELEMS = int64_t(1) << 29;
constexpr int CHAIN_MAX_KERNEL = 7;
// a * b, or CHAIN_MAX_ELEMS + 1 once it passes the bound (operands >= 0; no product overflows int64)
static int64_t chain_mul(int64_t a, int64_t b) {
    if (a > CHAIN_MAX_ELEMS || b > CHAIN_MAX_ELEMS) return CHAIN_MAX_ELEMS + 1;
    return std::min(a * b, CHAIN_MAX_ELEMS + 1);
}

// The shapes a layer list derives (the one rule niti_model_chain_check, niti_model_create_chain and
// build_chain share): per layer {c_in, c_out, k, pad, h_in, oh, out_h, flat_c}.  Refuses malformed
// lists and counts that do not fit an int; what else the library does not run is chain_check's.
// strided: the `3` entry points' rule, every layer at its own stride >= 1; else every layer is taken at
// stride 1, as the entry points that refuse any other stride always derived the shapes.
// A gpool layer (the `4` entry points' rule) leaves a 1x1 map of its c_out channels; a skip is checked for
// form against its source's output shape.
static int chain_shapes(const niti_chain_layer3* layers, int n, int in_c, int in_hw, bool strided,
                        std::vector<std::array<int, 8>>* out) {
    if (layers == nullptr || n < 1 || in_c < 1 || in_hw < 1) return NITI_INVALID_VALUE;
    int64_t c = in_c, h = in_hw;
    std::vector<std::array<int64_t, 2>> outs;  // per layer: the channels and map size the next layer sees
    for (int i = 0; i < n; ++i) {
        const niti_chain_layer3& l = layers[i];
        if (l.depthwise != 0 && l.depthwise != 1) return NITI_INVALID_VALUE;
        if (l.gpool != 0 && l.gpool != 1) return NITI_INVALID_VALUE;
        if (l.skip < 0 || l.skip > i) return NITI_INVALID_VALUE;
        // a depthwise layer has its input's channels: c_out 0 ("as the input") or that count
        if (l.depthwise && l.c_out != 0 && l.c_out != c) return NITI_INVALID_VALUE;
        const int64_t co = l.depthwise ? c : l.c_out;
        if (co < 1 || l.kernel < 1 || l.pad < 0 || l.pad >= l.kernel) return NITI_INVALID_VALUE;
        if (strided && l.stride < 1) return NITI_INVALID_VALUE;
        if (h + 2 * (int64_t)l.pad < l.kernel) return NITI_INVALID_VALUE;
        const int64_t oh = (h + 2 * (int64_t)l.pad - l.kernel) / (strided ? l.stride : 1) + 1;
        if (l.pool && oh < 2) return NITI_INVALID_VALUE;
        // a skip's source has the adding layer's conv output shape
        if (l.skip > 0 && (outs[i - l.skip][0] != co || outs[i - l.skip][1] != oh)) return NITI_INVALID_VALUE;
        const int64_t ph = l.pool ? (oh - 2) / 2 + 1 : oh;
        const int64_t fc = l.flatten ? chain_mul(chain_mul(co, ph), ph) : co;
        // (a count past int never reaches a buffer: refused here as a size no tensor of it fits)
        if (c > CHAIN_MAX_ELEMS || fc > CHAIN_MAX_ELEMS || oh > CHAIN_MAX_ELEMS) return NITI_NOT_SUPPORT;
        const bool one = l.flatten || l.gpool;
        if (out) out->push_back({(int)c, (int)co, l.kernel, l.pad, (int)h, (int)oh, (int)(one ? 1 : ph), (int)fc});
        c = fc;
        h = one ? 1 : ph;
        outs.push_back({c, h});
    }
    return NITI_NO_ERROR;
}

int chain_check(const niti_chain_layer3* layers, int n, int in_c, int in_hw, int batch, int shapes[][8], int rule) {
    std::vector<std::array<int, 8>> sh;
    const bool strided = rule >= CHAIN_RULE_STRIDED;
    if (batch < 1) return NITI_INVALID_VALUE;
    if (const int rc = chain_shapes(layers, n, in_c, in_hw, strided, &sh)) return rc;
    // (the update launch takes SGD_MAX_JOBS layers; the `4` entry points' lists update in groups of them)
    if (n > (rule >= CHAIN_RULE_WIDE ? NITI_CHAIN_MAX_LAYERS : SGD_MAX_JOBS)) return NITI_NOT_SUPPORT;
    for (int i = 0; i < n; ++i) {
        const niti_chain_layer3& l = layers[i];
        const std::array<int, 8>& s = sh[i];
        // the previous layer leaves a 1x1 map (a flatten or a global pool)
        const bool on_1x1 = i > 0 && (layers[i - 1].flatten || layers[i - 1].gpool);
        if (strided ? l.stride > 2 : l.stride != 1) return NITI_NOT_SUPPORT;
        // a strided layer after a flatten: its input is a 1x1 map
        if (l.stride != 1 && on_1x1) return NITI_NOT_SUPPORT;
        if (l.kernel > CHAIN_MAX_KERNEL) return NITI_NOT_SUPPORT;
        // a depthwise layer: not the first layer (its im2col form), not the logits, not on a flattened
        // map; the kernels take 3x3 and 5x5
        if (l.depthwise && (i == 0 || i == n - 1 || on_1x1 || (l.kernel != 3 && l.kernel != 5)))
            return NITI_NOT_SUPPORT;
        if (on_1x1 && (l.kernel != 1 || l.pad != 0)) return NITI_NOT_SUPPORT;
        if (l.skip != 0) {
            // a residual sum: not the logits; neither end on the 1x1 map behind a flatten or a global pool;
            // a source hands on its map as it is; the spans [i - skip, i] of two sums share at most an
            // endpoint (so no layer is the source of two)
            const int s = i - l.skip;
            const niti_chain_layer3& sl = layers[s];
            if (i == n - 1 || on_1x1 || (s > 0 && (layers[s - 1].flatten || layers[s - 1].gpool))) return NITI_NOT_SUPPORT;
            if (sl.pool || sl.flatten || sl.gpool) return NITI_NOT_SUPPORT;
            for (int j = s + 1; j < i; ++j)
                if (layers[j].skip != 0) return NITI_NOT_SUPPORT;
        }
        // a global pool: alone among pool / flatten, not the logits, int32 sums of at most 127 a pixel
        // (chain_mul saturates just past 2^29: the product below fits)
        if (l.gpool && (l.pool || l.flatten || i == n - 1 || chain_mul(s[5], s[5]) * 254 >= (int64_t(1) << 31)))
            return NITI_NOT_SUPPORT;
        // a first layer the fused input pass takes (input_im2col) stages kernel + band - 1 image rows
        // of 4 bytes a pixel in LDS: one output row must fit in half of a workgroup's 64 KiB
        // (a strided first layer does not run there)
        if (i == 0 && l.stride == 1 && Model::input_fused_ok(s[0], l.kernel, l.pad) &&
            (int64_t)l.kernel * (s[4] + l.kernel - 1) * 4 > 32768)
            return NITI_NOT_SUPPORT;
        if (i == n - 1 && (s[1] > 2048 || l.pool || l.flatten || s[5] != 1)) return NITI_NOT_SUPPORT;
        // every tensor of the layer, in the padded layouts build_chain allocates
        const int64_t b = batch, k2 = (int64_t)l.kernel * l.kernel;
        const int64_t cip32 = round_up(s[0], 32), cop32 = round_up(s[1], 32);
        const int64_t in_e = chain_mul(chain_mul(chain_mul(b, s[4]), s[4]), cip32);
        const int64_t out_e = chain_mul(chain_mul(chain_mul(b, s[5]), s[5]), cop32);
        const int64_t w_e = chain_mul(chain_mul(cop32, k2), cip32), flat_e = chain_mul(b, round_up(s[7], 16));
        if (in_e > CHAIN_MAX_ELEMS || out_e > CHAIN_MAX_ELEMS || w_e > CHAIN_MAX_ELEMS || flat_e > CHAIN_MAX_ELEMS)
            return NITI_NOT_SUPPORT;
    }
    if (shapes)
        for (int i = 0; i < n; ++i) std::copy(sh[i].begin(), sh[i].end(), shapes[i]);
    return NITI_NO_ERROR;
}

int Model::build(int arch_, int batch_, int in_hw) {
    // {c_out, kernel, stride, pad, relu, pool, flatten, depthwise, skip, gpool}
    std::vector<niti_chain_layer3> t;
    int ic = 3, hw = 32;
    if (arch_ == NITI_ARCH_LENET) {  // mnistTrain.cpp:131-181
        ic = 1;
        hw = 28;
        t = {{20, 5, 1, 0, 1, 1, 0, 0, 0, 0}, {52, 5, 1, 0, 1, 1, 1, 0, 0, 0}, {500, 1, 1, 0, 1, 0, 0, 0, 0, 0},
             {12, 1, 1, 0, 0, 0, 0, 0, 0, 0}};
    } else if (arch_ == NITI_ARCH_VGG11) {  // VGG-11 for 32x32 inputs, NITI layers (BASELINE cfg 3)
        static const int cfg[8][2] = {{64, 1}, {128, 1}, {256, 0}, {256, 1}, {512, 0}, {512, 1}, {512, 0}, {512, 1}};
        for (int i = 0; i < 8; ++i) t.push_back({cfg[i][0], 3, 1, 1, 1, cfg[i][1], 0, 0, 0, 0});
        t.push_back({12, 1, 1, 0, 0, 0, 0, 0, 0, 0});
    } else if (arch_ == NITI_ARCH_VGG16) {  // VGG-16 (configuration D), NITI layers (BASELINE cfg 4)
        hw = in_hw > 0 ? in_hw : 224;
        if (hw % 32 != 0) return NITI_INVALID_VALUE;
        static const int cfg[13][2] = {{64, 0},  {64, 1},  {128, 0}, {128, 1}, {256, 0}, {256, 0}, {256, 1},
                                       {512, 0}, {512, 0}, {512, 1}, {512, 0}, {512, 0}, {512, 1}};
        for (int i = 0; i < 13; ++i) t.push_back({cfg[i][0], 3, 1, 1, 1, cfg[i][1], /*flatten=*/i == 12, 0, 0, 0});
        t.push_back({4096, 1, 1, 0, 1, 0, 0, 0, 0, 0});
        t.push_back({4096, 1, 1, 0, 1, 0, 0, 0, 0, 0});
        t.push_back({1000, 1, 1, 0, 0, 0, 0, 0, 0, 0});
    } else {
        return NITI_NOT_SUPPORT;
    }
    return build_chain(arch_, batch_, t.data(), (int)t.size(), ic, hw, CHAIN_RULE_PLAIN);
}

int Model::build_chain(int arch_, int batch_, const niti_chain_layer3* layers, int nlayers, int in_c_, int in_hw,
                       int rule) {
    arch = arch_;
    batch = batch_;
    const bool strided = rule >= CHAIN_RULE_STRIDED;
    std::vector<std::array<int, 8>> sh;
    if (const int rc = chain_shapes(layers, nlayers, in_c_, in_hw, strided, &sh)) return rc;
    in_c = in_c_;
    in_h = in_w = in_hw;
    for (int i = 0; i < nlayers; ++i)
        add_conv(*this, sh[i][0], sh[i][1], sh[i][2], sh[i][3], sh[i][4], layers[i].relu != 0, layers[i].pool != 0,
                 layers[i].flatten != 0, layers[i].depthwise, strided ? layers[i].stride : 1, layers[i].gpool, layers[i].skip);
    for (const Layer& l : L)
        if (l.dw && !dwconv2_ok(l.g)) return NITI_NOT_SUPPORT;
    for (int i = 0; i < nlayers; ++i)
        if (L[i].skip) {
            L[i - L[i].skip].src_of = i;
            has_skip = true;
        }
    const int n = batch;
    {
        Layer& f = L[0];
        const ConvGeom o = f.og;
        if (o.c_in * o.kh * o.kw <= 32 && o.dh == 1 && o.dw == 1) {
            f.kp = 32;
            ConvGeom c{};
            c.n = o.n;
            c.c_in = 32;
            c.h = o.oh;
            c.w = o.ow;
            c.c_out = o.c_out;
            c.kh = c.kw = 1;
            c.sh = c.sw = 1;
            c.dh = c.dw = 1;
            c.finalize();
            f.g = c;
            f.xcol = (int8_t*)ws.alloc((size_t)n * o.oh * o.ow * 32);
            if (!f.xcol) return NITI_OUT_OF_MEMORY;
        }
    }
    x0 = (int8_t*)ws.alloc((size_t)n * in_h * in_w * round_up(in_c, 16));
    exp0 = (int8_t*)ws.alloc(16);
    size_t acc_elems = 0, sum_tmp_bytes = 0;
    const int nl = (int)L.size();
    // every layer's int32 weight gradient in one contiguous bucket: data parallel, one SUM
    // all-reduce covers the whole step's gradients
    size_t grad_elems = 0;
    for (const Layer& l : L) grad_elems += (size_t)l.w_elems();
    grad_bucket = (int32_t*)ws.alloc(grad_elems * 4);
    if (!grad_bucket) return NITI_OUT_OF_MEMORY;
    grad_bucket_elems = grad_elems;
    size_t grad_off = 0;
    sgd_jobs.assign(nl, SgdJob{});
    sgd_many.assign(nl, SgdJob{});
    xp16.assign(nl, nullptr);
    xp16_valid.assign(nl, 0);
    dp16.assign(nl, nullptr);
    dp16_valid.assign(nl, 0);
    xc32_valid.assign(nl, 0);
    dyc32_valid.assign(nl, 0);
    dy16_valid.assign(nl, 1);
    rc_err = (uint32_t*)ws.alloc(64);
    if (!rc_err || hipMemset(rc_err, 0, 64) != hipSuccess) return NITI_OUT_OF_MEMORY;
    for (int i = 0; i < nl; ++i) {
        Layer& l = L[i];
        const ConvGeom& g = l.g;
        const size_t out_px = (size_t)n * g.oh * g.ow;
        l.w = (int8_t*)ws.alloc(l.w_elems());
        l.ws_dev = (int8_t*)ws.alloc(16);
        l.wT = (int8_t*)ws.alloc((size_t)g.c_in * g.kh * g.kw * g.cop);
        l.r = (int8_t*)ws.alloc(out_px * g.cop);
        if (l.pool) {
            l.p = (int8_t*)ws.alloc((size_t)n * l.ph * l.pw * g.cop);
            l.dtmp = (int8_t*)ws.alloc((size_t)n * l.ph * l.pw * g.cop);
            if (!l.p || !l.dtmp) return NITI_OUT_OF_MEMORY;
            if (!l.flatten && l.ph * 2 == g.oh && l.pw * 2 == g.ow) {
                l.pc = (int8_t*)ws.alloc((size_t)n * l.ph * l.pw * g.cop);
                if (!l.pc) return NITI_OUT_OF_MEMORY;
            }
        }
        if (l.flatten) {
            const int fc = g.c_out * l.fh() * l.fw();
            l.flat = (int8_t*)ws.alloc((size_t)n * round_up(fc, 16));
            l.dflat = (int8_t*)ws.alloc((size_t)n * round_up(fc, 16));
            // without a pool the flatten's gradient lands on the conv output's own map, ahead of
            // the relu gradient
            if (!l.pool) l.dtmp = (int8_t*)ws.alloc(out_px * g.cop);
            if (!l.flat || !l.dflat || !l.dtmp) return NITI_OUT_OF_MEMORY;
        }
        if (l.gpool) {  // the sums, the pooled map and its gradient [n][cop], the pooled exponent
            l.gsum = (int32_t*)ws.alloc((size_t)n * g.cop * 4);
            l.flat = (int8_t*)ws.alloc((size_t)n * g.cop);
            l.dflat = (int8_t*)ws.alloc((size_t)n * g.cop);
            l.exp_gp = (int8_t*)ws.alloc(16);
            if (!l.gsum || !l.flat || !l.dflat || !l.exp_gp) return NITI_OUT_OF_MEMORY;
        }
        l.dy = (int8_t*)ws.alloc(out_px * g.cop);
        l.dwacc = grad_bucket + grad_off;
        grad_off += (size_t)l.w_elems();
        l.g8 = (int8_t*)ws.alloc(l.w_elems());
        l.exp = (int8_t*)ws.alloc(16);
        l.gspec = (uint32_t*)ws.alloc(2 * GEMM_SPEC_SLOT_WORDS * 4);
        if (!l.w || !l.ws_dev || !l.wT || !l.r || !l.dy || !l.dwacc || !l.g8 || !l.exp || !l.gspec)
            return NITI_OUT_OF_MEMORY;
        if (hipMemset(l.gspec, 0, 2 * GEMM_SPEC_SLOT_WORDS * 4) != hipSuccess) return NITI_NO_EXECUTION;
        if (hipMemset(l.w, 0, l.w_elems()) != hipSuccess) return NITI_NO_EXECUTION;
        if (hipMemset(l.ws_dev, 0, 16) != hipSuccess) return NITI_NO_EXECUTION;
        acc_elems = std::max(acc_elems, out_px * g.cop);
        acc_elems = std::max(acc_elems, (size_t)n * g.h * g.w * g.cip);
        slab_bytes = std::max(slab_bytes, conv_fwd_workspace(g));
        slab_bytes = std::max(slab_bytes, conv_dgrad_workspace(g));
        slab_w_bytes = std::max(slab_w_bytes, conv_wgrad_workspace(g));
        // grid-barrier state of every layer: the row kernels' fused launches and speculation slots,
        // the head's, or the GEMM path's fused-rescale launches (STRAT_FUSED)
        l.bar = (uint32_t*)ws.alloc(ROWCONV_BAR_WORDS * 4);
        if (!l.bar || hipMemset(l.bar, 0, ROWCONV_BAR_WORDS * 4) != hipSuccess) return NITI_OUT_OF_MEMORY;
        if (l.dw) {  // its weight gradient's slabs: the layer's own until the update (the deferred combine)
            l.slab16_bytes = (size_t)dwconv_wgrad_slabs(g) * l.w_elems() * sizeof(int32_t);
            l.slab16 = (int32_t*)ws.alloc(l.slab16_bytes);
            if (!l.slab16) return NITI_OUT_OF_MEMORY;
        }
        if (i > 0 && !l.dw && conv_dgrad_subpix_ok(g)) {
            l.subw = (int8_t*)ws.alloc(conv_dgrad_subpix_bytes(g));
            if (!l.subw) return NITI_OUT_OF_MEMORY;
        }
        if (has_skip) {
            l.edy = (int8_t*)ws.alloc(16);
            if (!l.edy || hipMemset(l.edy, 0, 16) != hipSuccess) return NITI_OUT_OF_MEMORY;
        }
        if (l.skip) {
            l.ey = (int8_t*)ws.alloc(16);
            if (!l.ey) return NITI_OUT_OF_MEMORY;
            sum_tmp_bytes = std::max(sum_tmp_bytes, out_px * g.cop);
        }
        if (!l.kp && !l.dw && !l.skip && rowconv_ok(g)) {
            l.rc = 1;
            l.wf = (int8_t*)ws.alloc(rowconv_wf_bytes(g.c_out, g.c_in));
            l.xc32 = (int8_t*)ws.alloc((size_t)n * round_up(g.c_in, 32) * g.h * g.w);
            if (!l.wf || !l.xc32) return NITI_OUT_OF_MEMORY;
            if (hipMemset(l.wf, 0, rowconv_wf_bytes(g.c_out, g.c_in)) != hipSuccess)
                return NITI_NO_EXECUTION;
            rc_acc_size = std::max(rc_acc_size, rowconv_acc_bytes(g, false));
            // the input gradient too, where the previous layer's output (pooled 2x2 or not) is
            // this layer's input as is
            const Layer* pv = i > 0 ? &L[i - 1] : nullptr;
            const bool pv_ok = pv != nullptr && !pv->to_1x1() && pv->src_of < 0 && pv->g.cop == g.cip &&
                               (pv->pool ? (pv->ph == g.h && pv->pw == g.w && pv->g.oh == 2 * g.h && pv->g.ow == 2 * g.w)
                                         : (pv->g.oh == g.h && pv->g.ow == g.w));
            if (pv_ok && rowconv_dgrad_geom(g, &l.dg)) {
                l.rcd = 1;
                rc_acc_size = std::max(rc_acc_size, rowconv_acc_bytes(l.dg, true, pv->pool != 0));
                l.wft = (int8_t*)ws.alloc(rowconv_wf_bytes(g.c_in, g.c_out));
                l.dyc32 = (int8_t*)ws.alloc(out_px * round_up(g.c_out, 32));
                if (!l.wft || !l.dyc32) return NITI_OUT_OF_MEMORY;
                if (hipMemset(l.wft, 0, rowconv_wf_bytes(g.c_in, g.c_out)) != hipSuccess) return NITI_NO_EXECUTION;
            }
        }
        if (!l.dw && conv_wgrad_p16_ok(g)) {
            slab_w_bytes = std::max(slab_w_bytes, conv_wgrad_p16_workspace(g, 8));
            xp16[i] = (int8_t*)ws.alloc((size_t)n * g.h * g.w * g.cip);
            l.slab16_bytes = conv_wgrad_p16_workspace(g, 8);
            l.slab16 = l.slab16_bytes ? (int32_t*)ws.alloc(l.slab16_bytes) : nullptr;
            if (l.slab16_bytes && !l.slab16) return NITI_OUT_OF_MEMORY;
            dp16[i] = (int8_t*)ws.alloc(out_px * g.cop);
            if (!xp16[i] || !dp16[i]) return NITI_OUT_OF_MEMORY;
        }
        // layer input / its C alignment with the previous output
        if (i == 0) {
            l.in = l.kp ? l.xcol : x0;
        } else {
            const Layer& pr = L[i - 1];
            l.in = pr.to_1x1() ? pr.flat : (pr.pool ? pr.p : pr.r);
        }
    }
    acc = (int32_t*)ws.alloc(acc_elems * 4);
    qstats = (unsigned long long*)ws.alloc(64);
    qslots = (unsigned long long*)ws.alloc((size_t)IMAGE_STATS_SLOTS * 4 * sizeof(unsigned long long));
    x0n = (int8_t*)ws.alloc((size_t)n * in_c * in_h * in_w);
    if (!qstats || !qslots || !x0n) return NITI_OUT_OF_MEMORY;
    if (slab_bytes) {
        slab = ws.alloc(slab_bytes);
        if (!slab) return NITI_OUT_OF_MEMORY;
    }
    if (slab_w_bytes) {
        slab_w = ws.alloc(slab_w_bytes);
        if (!slab_w) return NITI_OUT_OF_MEMORY;
    }
    if (rc_acc_size) {
        rc_acc = (int32_t*)ws.alloc(rc_acc_size);
        if (!rc_acc) return NITI_OUT_OF_MEMORY;
    }
    if (nl >= 2 && L[0].kp && L[0].pc != nullptr &&
        conv0_wgrad_codes_ok(L[0].g.n, L[0].g.oh, L[0].g.ow, L[0].g.cop, L[0].g.cip)) {
        c0w_slab_bytes = (size_t)conv0_wgrad_codes_blocks(L[0].g.n, L[0].g.oh, L[0].g.ow, 1 << 30) * L[0].g.cop * 32 * 4;
        c0w_slab = (int32_t*)ws.alloc(c0w_slab_bytes);
        if (!c0w_slab) return NITI_OUT_OF_MEMORY;
    }
    for (int i = 0; i < nl; ++i) {  // the GEMM-path phases that may run the speculative pair
        const Layer& l = L[i];
        if (!(l.kp && conv0_ok(l.g)) && !l.rc) gspec_alt_bytes = std::max(gspec_alt_bytes, conv_fwd_spec_alt_bytes(l.g));
        if (i > 0 && !l.rcd) gspec_alt_bytes = std::max(gspec_alt_bytes, conv_dgrad_spec_alt_bytes(l.g));
    }
    if (gspec_alt_bytes && !(gspec_alt = (int8_t*)ws.alloc(gspec_alt_bytes))) return NITI_OUT_OF_MEMORY;
    // (a global pool's range: one more word set per gpool layer, behind the layers' three each)
    // (and a residual sum's: one per adding layer, one per source)
    int n_gp = 0;
    for (const Layer& l : L) n_gp += l.gpool + (l.skip ? 2 : 0);
    amax_bytes = (size_t)(3 * nl + n_gp) * MAX_BYTES;
    amax = (uint32_t*)ws.alloc(amax_bytes);
    for (int i = 0, k = 0; i < nl && amax != nullptr; ++i) {
        if (L[i].gpool) L[i].gp_amax = amax + (size_t)(3 * nl + k++) * MAX_WORDS;
        if (L[i].skip) {
            L[i].sum_amax = amax + (size_t)(3 * nl + k++) * MAX_WORDS;
            L[i - L[i].skip].bsum_amax = amax + (size_t)(3 * nl + k++) * MAX_WORDS;
        }
    }
    if (has_skip) {
        sum_tmp = (int8_t*)ws.alloc(sum_tmp_bytes);
        e_tmp = (int8_t*)ws.alloc(16);
        if (!sum_tmp || !e_tmp) return NITI_OUT_OF_MEMORY;
    }
    if (!x0 || !exp0 || !acc || !amax) return NITI_OUT_OF_MEMORY;
    // L has its final size: the base's view of the layers (ahead of alloc_update_bits, which counts them)
    for (int i = 0; i < nl; ++i) {
        L[i].wg_amax = rng(i, 2);
        P.push_back(&L[i]);
    }
    if (const int rc = alloc_eval()) return rc;
    if (const int rc = alloc_update_bits()) return rc;
    if (hipMemset(x0, 0, (size_t)n * in_h * in_w * round_up(in_c, 16)) != hipSuccess) return NITI_NO_EXECUTION;
    return hipDeviceSynchronize() == hipSuccess ? NITI_NO_ERROR : NITI_NO_EXECUTION;
}

int Model::step(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st) {
    // (the batched weight gradient's table: rebuilt here, never inside run() or a capture)
    if (const int rc = build_wgrad_batch(wgrad_batch_t())) return rc;
    if (!use_graph || coll != nullptr) return run(x_nchw, exp_in, images, labels, st);
    Key k;
    k.x = x_nchw ? (const void*)x_nchw : (const void*)images;
    k.labels = labels;
    k.exp_in = exp_in;
    k.pl = probe_layer;
    k.pp = probe_phase;
    if (segs.empty() || !(k == key)) {
        drop_graph();
        if (const int rc = ensure_graph_stream()) return rc;
        DTRY(hipStreamBeginCapture(gstream, hipStreamCaptureModeThreadLocal));
        capturing = true;
        cap_err = hipSuccess;
        const int rc = run(x_nchw, exp_in, images, labels, gstream);
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamEndCapture(gstream, &g);
        capturing = false;
        hipGraphExec_t ex = nullptr;
        if (e == hipSuccess && rc == NITI_NO_ERROR) e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
        if (g) (void)hipGraphDestroy(g);
        if (e == hipSuccess && rc == NITI_NO_ERROR) segs.push_back(ex);
        if (rc != NITI_NO_ERROR || e != hipSuccess || cap_err != hipSuccess || (segs.size() != 1 && segs.size() != 3)) {
            drop_graph();
            use_graph = false;  // fall back to direct launches for this model
            (void)hipGetLastError();
            return run(x_nchw, exp_in, images, labels, st);
        }
        key = k;
    }
    DTRY(hipEventRecord(gin, st));
    DTRY(hipStreamWaitEvent(gstream, gin, 0));
    const bool probing = segs.size() == 3 && !probe_paused && probe_count < (int)ev0.size();
    for (size_t j = 0; j < segs.size(); ++j) {
        if (probing && j == 1) DTRY(hipEventRecord(ev0[probe_count], gstream));
        if (probing && j == 2) DTRY(hipEventRecord(ev1[probe_count++], gstream));
        DTRY(hipGraphLaunch(segs[j], gstream));
    }
    DTRY(hipEventRecord(gout, gstream));
    DTRY(hipStreamWaitEvent(st, gout, 0));
    return NITI_NO_ERROR;
}

// One layer's forward: GEMM range pass -> [all-reduce MAX] -> requantise (+relu, fused pool
// when the requant is a separate pass) -> pool / flatten.
int Model::fwd_layer(int i, hipStream_t st) {
    const int rc = fwd_conv_layer(i, st);
    if (rc != NITI_NO_ERROR || !L[i].gpool) return rc;
    return gpool_fwd(i, st);
}

// The global sum pool of layer i's output: the sums and their range, [all-reduce MAX], the forward rule's
// requantisation into the 1x1 map the next layer reads (exponent e + inc).
int Model::gpool_fwd(int i, hipStream_t st) {
    Layer& l = L[i];
    const ConvGeom& g = l.g;
    DTRY(sum_pool_wide(l.r, batch, g.oh * g.ow, g.cop, l.gsum, l.gp_amax, st));
    DTRY(range_max(l.gp_amax, st));
    ActRequant r;
    r.acc = l.gsum;
    r.rows = batch;
    r.ldc = g.cop;
    r.amax = l.gp_amax;
    r.exp_in = l.exp;
    r.exp_out = l.exp_gp;
    r.out_nhwc16 = l.flat;
    DTRY(requant_act(r, st));
    return NITI_NO_ERROR;
}

// The residual sum of adding layer i (niti_resnet.hip's two launches: the range of the aligned sum,
// [all-reduce MAX], the sum recomputed and requantised): conv output (operand a) + the source's final
// output -> r, with the layer's relu; the layer's exponent is e_z + inc.
int Model::skip_sum_fwd(int i, hipStream_t st) {
    Layer& l = L[i];
    const Layer& s = L[i - l.skip];
    const int64_t n = (int64_t)batch * l.g.oh * l.g.ow * l.g.cop;
    DTRY(residual_add(sum_tmp, l.ey, s.r, s.exp, n, nullptr, nullptr, l.sum_amax, st));
    DTRY(range_max(l.sum_amax, st));
    DTRY(residual_requant(sum_tmp, l.ey, s.r, s.exp, n, l.sum_amax, nullptr, l.exp, l.relu, l.r, st));
    return NITI_NO_ERROR;
}

// The gradient sum at source s: layer s + 1's unmasked input gradient (operand a: sum_tmp, exponent e_tmp)
// + the adding layer's output gradient -> the source's dy through its own relu mask, exponent e_z + inc.
int Model::skip_sum_bwd(int si, hipStream_t st) {
    Layer& s = L[si];
    const Layer& a = L[s.src_of];
    const int64_t n = (int64_t)batch * s.g.oh * s.g.ow * s.g.cop;
    DTRY(residual_add(sum_tmp, e_tmp, a.dy, a.edy, n, nullptr, nullptr, s.bsum_amax, st));
    DTRY(range_max(s.bsum_amax, st));
    DTRY(residual_requant(sum_tmp, e_tmp, a.dy, a.edy, n, s.bsum_amax, nullptr, s.edy, 0, s.dy, st, s.relu ? s.r : nullptr));
    return NITI_NO_ERROR;
}

int Model::fwd_conv_layer(int i, hipStream_t st) {
    const int n = batch;
    const bool dp = this->dp();
    Layer& l = L[i];
    const ConvGeom& g = l.g;
    auto flatten_fwd = [&] {  // the NCHW flatten of the (pooled) output
        const int ld = round_up(g.c_out * l.fh() * l.fw(), 16);
        return launch_map((int64_t)n * ld, FlattenFwd{l.fsrc(), l.fh() * l.fw(), g.c_out, g.cop, ld, l.flat}, st);
    };
    probe(i, 0, true, st);
    l.r_written = true;
    if (l.kp && conv0_ok(g) && !l.flatten) {
        // first layer on its im2col copy: range pass, [all-reduce MAX], requant + relu + pool pass
        ActOut o;
        const bool code = pool_code_layer(i);
        l.r_written = keep_grads || !code;
        o.out = l.r_written ? l.r : nullptr;
        o.relu = l.relu;
        o.exp_in = exp0;
        o.wscale = l.ws_dev;
        o.exp_out = l.exp;
        o.pool.pool_out = l.pool ? l.p : nullptr;
        // the (pooled) output also as the next layer's C32 input when it runs on the row kernel
        const bool next_c32 = i + 1 < (int)L.size() && rowconv_layer(i + 1) && !rowconv_nhwc_pref(L[i + 1].g);
        if (!conv0_ranged) DTRY(conv0_fwd(g, l.in, l.w, rng(i, 0), o, 0, st));
        conv0_ranged = false;
        DTRY(range_max(rng(i, 0), st));
        DTRY(conv0_fwd(g, l.in, l.w, rng(i, 0), o, 1, st, next_c32 && l.pool ? L[i + 1].xc32 : nullptr,
                       next_c32 && !l.pool ? L[i + 1].xc32 : nullptr, code ? l.pc : nullptr));
        if (next_c32) xc32_valid[i + 1] = 1;
        probe(i, 0, false, st);
        return NITI_NO_ERROR;
    }
    if (head_layer(i)) {
        // the classifier head on the row kernel (W = 1): one fused launch, or range + requantise
        RowConvOut o;
        o.out = l.r;
        o.exp_in = i == 0 ? exp0 : L[i - 1].oexp();
        o.wscale = l.ws_dev;
        o.exp_out = l.exp;
        o.relu = l.relu;
        const int K = g.c_in, rows = g.c_out;
        const int rc = rowconv_ranged(rowconv_fc_ok(n, K, rows, true), false, o, rng(i, 0), l.bar, l.epoch, st,
                                      [&](const RowConvOut& ro, int mode, uint32_t* bar, uint32_t epoch, uint32_t* err) {
                                          return rowconv_fc(n, K, rows, l.in, g.cip, l.w, g.cip, ro, mode, rng(i, 0), bar,
                                                            epoch, err, st);
                                      });
        if (rc != NITI_NO_ERROR) return rc;
        probe(i, 0, false, st);
        return NITI_NO_ERROR;
    }
    if (rowconv_layer(i)) {
        // register-fed forward, rescale fused: one launch with an in-kernel grid barrier (single
        // device, every workgroup resident, not inside a graph capture), else a range launch,
        // [all-reduce MAX], and a recompute-and-requantise launch
        // a row-segment layer reads its NHWC16 input in place; the others their C32 copy
        const bool xn = rowconv_nhwc_pref(g);
        if (!xn && !xc32_valid[i]) {
            DTRY(nhwc16_to_c32(l.in, n, g.h * g.w, g.cip, g.c_in, l.xc32, st));
            xc32_valid[i] = 1;
        }
        const int8_t* xin = xn ? l.in : l.xc32;
        RowConvOut o;
        o.x_nhwc = xn ? 1 : 0;
        const bool code = pool_code_layer(i);
        l.r_written = keep_grads || !code;
        o.out = l.r_written ? l.r : nullptr;
        o.pool_out = l.pool ? l.p : nullptr;
        o.pool_code_out = code ? l.pc : nullptr;
        const bool feeds_next = i + 1 < (int)L.size() && rowconv_layer(i + 1) && !l.to_1x1() &&
                                !rowconv_nhwc_pref(L[i + 1].g);
        o.next = feeds_next ? L[i + 1].xc32 : nullptr;
        o.exp_in = i == 0 ? exp0 : L[i - 1].oexp();
        o.wscale = l.ws_dev;
        o.exp_out = l.exp;
        o.relu = l.relu;
        const int rc = rowconv_ranged(rowconv_fused_ok(g), rowconv_acc_bytes(g, false) != 0, o, rng(i, 0), l.bar, l.epoch,
                                      st, [&](const RowConvOut& ro, int mode, uint32_t* bar, uint32_t epoch, uint32_t* err) {
                                          return rowconv_fwd(g, xin, l.wf, ro, mode, rng(i, 0), bar, epoch, err, st);
                                      });
        if (rc != NITI_NO_ERROR) return rc;
        if (feeds_next) xc32_valid[i + 1] = 1;
        probe(i, 0, false, st);
        if (l.flatten) DTRY(flatten_fwd());
        return NITI_NO_ERROR;
    }
    // (an adding layer: the requantised conv output waits in sum_tmp, linear, for its sum)
    ActOut o;
    o.out = l.skip ? sum_tmp : l.r;
    o.relu = l.skip ? 0 : l.relu;
    o.exp_in = i == 0 ? exp0 : L[i - 1].oexp();
    o.wscale = l.ws_dev;
    o.exp_out = l.skip ? l.ey : l.exp;
    if (l.dw) {
        // depthwise: range launch, [all-reduce MAX], recompute-and-requantise launch; the unfused pool / flatten
        const auto none = [](const ActOut&, auto) { return hipErrorNotSupported; };
        const int rc = gemm_ranged(false, false, o, rng(i, 0), l.bar, l.epoch, st, none, none, [&](const ActOut& ao, int ph) {
            return dwconv_fwd(g, l.in, l.w, rng(i, 0), ao, ph - 1, st);
        });
        if (rc != NITI_NO_ERROR) return rc;
        probe(i, 0, false, st);
        if (l.skip)
            if (const int rs = skip_sum_fwd(i, st)) return rs;
        if (l.pool) DTRY(maxpool_nhwc16(l.r, n, g.oh, g.ow, g.cop, 2, 2, 0, l.p, l.ph, l.pw, st));
        if (l.flatten) DTRY(flatten_fwd());
        return NITI_NO_ERROR;
    }
    const bool spec = conv_fwd_spec_ok(g);
    // the 2x2 pool rides along the separate requant pass when there is one
    const bool fuse_pool = !spec && l.pool && !l.skip && g.oh % 2 == 0 && g.ow % 2 == 0 && conv_fwd_phase2_separate(g, slab_bytes);
    if (fuse_pool) {
        o.pool.pool_out = l.p;
        o.pool.H = g.oh;
        o.pool.W = g.ow;
    }
    // (the pair: one GEMM pass while the bit width holds, no int32 tensor)
    const int rc = gemm_ranged(
        !dp && !capturing && !fuse_pool, spec, o, rng(i, 0), l.bar, l.epoch, st,
        [&](const ActOut& ao, const FusedBar& fb) { return conv_fwd_fused(g, l.in, l.w, ao, fb, st); },
        [&](const ActOut& ao, int ph) {
            int8_t* alt = conv_fwd_spec_alt_bytes(g) <= gspec_alt_bytes ? gspec_alt : nullptr;
            return conv_fwd_spec(g, l.in, l.w, rng(i, 0), ao, l.gspec, ph, st, alt);
        },
        [&](const ActOut& ao, int ph) {
            return ph == 1 ? conv_fwd_phase1(g, l.in, l.w, acc, rng(i, 0), slab, slab_bytes, st)
                           : conv_fwd_phase2(g, l.in, l.w, acc, rng(i, 0), ao, slab_bytes, st);
        });
    if (rc != NITI_NO_ERROR) return rc;
    probe(i, 0, false, st);
    if (l.skip)
        if (const int rs = skip_sum_fwd(i, st)) return rs;
    if (l.pool && !fuse_pool) DTRY(maxpool_nhwc16(l.r, n, g.oh, g.ow, g.cop, 2, 2, 0, l.p, l.ph, l.pw, st));
    if (l.flatten) DTRY(flatten_fwd());
    return NITI_NO_ERROR;
}

// One layer's weight gradient (the int32 gradient and, single device, its range; data
// parallel, the SUM and the range follow on the comm stream in sum_bucket).
int Model::wgrad_layer(int i, hipStream_t st) {
    const bool dp = this->dp();
    Layer& l = L[i];
    const ConvGeom& g = l.g;
    if (head_layer(i) && g.c_out <= 32 && g.cip % 32 == 0) {
        // the classifier head: one small launch, its range published (single device)
        probe(i, 2, true, st);
        DTRY(head_wgrad(g.n, g.c_out, g.cip, l.in, g.cip, l.dy, g.cop, l.dwacc, dp ? nullptr : rng(i, 2), st));
        probe(i, 2, false, st);
        return NITI_NO_ERROR;
    }
    l.fc_sgd = fc_sgd_layer(i);
    SgdJob& defer_job = L[i].defer;
    if (l.dw) {
        // depthwise: one launch leaves C-shaped slabs; single device they go to the update launch's
        // combine, else (data parallel, a capture, the combine off) they are reduced here with the range
        probe(i, 2, true, st);
        int slabs = 0;
        defer_job = SgdJob{};
        SgdJob d{};
        DTRY(dwconv_wgrad(g, l.in, l.dy, l.slab16, l.slab16_bytes, &slabs, st, &d));
        if (defer_combine())
            defer_job = d;
        else
            DTRY(splitk_reduce_linear(l.slab16, slabs, l.w_elems(), d.slab_stride, l.dwacc, dp ? nullptr : rng(i, 2), st));
        probe(i, 2, false, st);
        return NITI_NO_ERROR;
    }
    if (i == 0 && conv0_codes_route()) {
        // from g0 (the first quarter of dy, left by layer 1's input gradient), the codes and xcol; the
        // slabs go to the update launch's combine, as the GEMM path's do (wgrad_gemm)
        int slabs = 0;
        defer_job = SgdJob{};
        DTRY(conv0_wgrad_codes(g.n, g.oh, g.ow, g.cop, g.cip, l.dy, l.pc, l.xcol, conv0_wgrad_codes_model_blocks(),
                               c0w_slab, c0w_slab_bytes, &slabs, st));
        ++g_c0w_launches;
        SgdJob d{};
        d.slab = c0w_slab;
        d.splits = slabs;
        d.slab_stride = (int64_t)g.cop * 32;
        d.slab_n = l.w_elems();
        if (defer_combine()) {
            defer_job = d;
        } else if (tuning && in_step_combine()) {  // (timed with the combine the step runs it with)
            d.acc = l.dwacc;
            d.amax = rng(i, 2);
            DTRY(sgd_combine_many(&d, 1, st));
        } else {
            DTRY(splitk_reduce_linear(c0w_slab, slabs, l.w_elems(), d.slab_stride, l.dwacc, dp ? nullptr : rng(i, 2), st));
        }
        return NITI_NO_ERROR;
    }
    if (l.fc_sgd) {  // its range now; the recompute with the update after the backward pass
        defer_job = SgdJob{};
        DTRY(conv_wgrad_fc_sgd(g, l.in, l.dy, rng(i, 2), SgdJob{}, 0, st));
        return NITI_NO_ERROR;
    }
    if (const int s = wgrad_p16_splits(i)) {
        // P16 weight gradient: x (unless run() converted every input already) and dy to pixel
        // blocks, then the register-fed kernel (+ its split-K reduce); the probe times the kernel
        // launch itself
        if (!xp16_valid[i]) {
            DTRY(nhwc16_to_p16(l.in, (int64_t)g.n * g.h * g.w, g.cip, xp16[i], st));
            xp16_valid[i] = 1;
        }
        if (!dp16_valid[i]) {
            DTRY(nhwc16_to_p16(l.dy, (int64_t)g.n * g.oh * g.ow, g.cop, dp16[i], st));
            dp16_valid[i] = 1;
        }
        hipEvent_t eb, ee;
        unsigned long long* sp;
        probe_launch(i, 2, &eb, &ee, &sp);
        // single device: the split-K combine (+ range) runs with every other layer's in one launch
        // ahead of NITI_SGD, over this layer's own slabs (the shared workspace is reused by the
        // next layer)
        const bool defer = defer_combine() && s > 1 && l.slab16 != nullptr &&
                           conv_wgrad_p16_workspace(g, s) <= l.slab16_bytes;
        defer_job = SgdJob{};
        DTRY(conv_wgrad_p16(g, xp16[i], dp16[i], l.dwacc, dp ? nullptr : rng(i, 2), defer ? l.slab16 : slab_w,
                            defer ? l.slab16_bytes : slab_w_bytes, s, st, eb, ee, sp, defer ? &defer_job : nullptr));
        return NITI_NO_ERROR;
    }
    // the weight-gradient probe is the GEMM launch's own begin / end (its split-K reduce excluded)
    if (capturing)
        probe(i, 2, true, st);
    else
        arm_kernel_events(i, 2);
    arm_span(i, 2);
    return wgrad_gemm(i, l.in, l.dy, capturing ? probe_end_event(i, 2) : nullptr, st);
}

// Input gradient of layer i (i > 0) into the previous layer's output gradient, with the
// previous layer's pool / flatten / relu gradients.
int Model::dgrad_layer(int i, hipStream_t st) {
    const int n = batch;
    const bool dp = this->dp();
    Layer& l = L[i];
    const ConvGeom& g = l.g;
    Layer& pv = L[i - 1];
    probe(i, 1, true, st);
    if (head_dgrad_ok(i)) {
        // the head's input gradient on the row kernel (W = 1), into the previous layer's relu or
        // 2x2-pool gradient (+ its C32 / P16 copies)
        RowConvOut o;
        o.dgrad_slot = 1;  // (every input-gradient launch: its own speculation hint slot)
        int8_t* next = rowconv_dgrad_layer(i - 1) && !rowconv_nhwc_pref(pv.dg) ? pv.dyc32 : nullptr;
        if (pv.pool) {
            if (pool_code_layer(i - 1)) {
                o.pool_code = pv.pc;
            } else {
                o.pool_x = pv.r;
                o.pool_y = pv.p;
            }
            o.pool_dx = pv.dy;
            o.pool_dx_next = next;
            o.pool_relu = pv.relu;
            o.p16 = fuse_dp16 && wgrad_p16_splits(i - 1) > 0 && (4 * n) % 16 == 0 ? dp16[i - 1] : nullptr;
            o.pool_dx_nhwc = skip_dy16(i, next, o.p16) ? 0 : 1;
        } else {
            o.out = pv.dy;
            o.relu_mask = pv.relu ? pv.r : nullptr;
            next = nullptr;  // a 1x1 previous layer has no row-kernel input gradient
        }
        if (has_skip) {  // the gradient's exponent travels with it: e_dy + wscale + inc
            o.exp_in = l.edy;
            o.wscale = l.ws_dev;
            o.exp_out = pv.edy;
        }
        dy16_valid[i - 1] = !(pv.pool && o.pool_dx_nhwc == 0);
        const int K = g.c_out, rows = g.c_in;
        const int rc = rowconv_ranged(rowconv_fc_ok(n, K, rows, true), false, o, rng(i, 1), l.bar, l.epoch, st,
                                      [&](const RowConvOut& ro, int mode, uint32_t* bar, uint32_t epoch, uint32_t* err) {
                                          return rowconv_fc(n, K, rows, l.dy, g.cop, l.wT, g.cop, ro, mode, rng(i, 1), bar,
                                                            epoch, err, st);
                                      });
        if (rc != NITI_NO_ERROR) return rc;
        probe(i, 1, false, st);
        dp16_valid[i - 1] = o.p16 != nullptr ? 1 : 0;
        dyc32_valid[i - 1] = next != nullptr ? 1 : 0;
        return NITI_NO_ERROR;
    }
    if (rowconv_dgrad_layer(i)) {
        // register-fed input gradient, its requantisation and the previous layer's relu / pool
        // gradient fused; the previous layer's dy also in C32 when its own input gradient runs here
        const ConvGeom& d = l.dg;
        // a row-segment input gradient reads dy (NHWC16) in place; the others its C32 copy
        const bool xn = rowconv_nhwc_pref(d);
        if (xn && !dy16_valid[i]) DTRY(c32_to_nhwc16(l.dyc32, n, g.oh * g.ow, g.cop, g.c_out, l.dy, st));
        if (!xn && !dyc32_valid[i]) {
            DTRY(nhwc16_to_c32(l.dy, n, g.oh * g.ow, g.cop, g.c_out, l.dyc32, st));
            dyc32_valid[i] = 1;
        }
        const int8_t* dyin = xn ? l.dy : l.dyc32;
        RowConvOut o;
        o.dgrad_slot = 1;  // (every input-gradient launch: its own speculation hint slot)
        o.x_nhwc = xn ? 1 : 0;
        int8_t* next = rowconv_dgrad_layer(i - 1) && !rowconv_nhwc_pref(pv.dg) ? pv.dyc32 : nullptr;
        // the previous layer's P16 dy for its weight gradient, when the launch's pixels make whole
        // 16-pixel blocks; else wgrad_layer converts
        o.p16 = fuse_dp16 && wgrad_p16_splits(i - 1) > 0 && rowconv_p16_ok(l.dg, pv.pool) ? dp16[i - 1] : nullptr;
        const bool skip16 = skip_dy16(i, next, o.p16);
        // layer 0 on the codes route: the plain epilogue, q of every pooled pixel into the first
        // quarter of its dy (the launch then has no input-gradient operand: the forward instantiation)
        const bool g0_only = i == 1 && conv0_codes_route();
        if (i == 1) dy0_codes = g0_only;
        if (g0_only) {
            o.out = pv.dy;
            o.p16 = nullptr;
            next = nullptr;
        } else if (pv.pool) {
            if (pool_code_layer(i - 1)) {
                o.pool_code = pv.pc;
            } else {
                o.pool_x = pv.r;
                o.pool_y = pv.p;
            }
            o.pool_dx = pv.dy;
            o.pool_dx_next = next;
            o.pool_relu = pv.relu;
            o.pool_dx_nhwc = skip16 ? 0 : 1;
        } else {
            o.out = skip16 ? nullptr : pv.dy;
            o.next = next;
            o.relu_mask = pv.relu ? pv.r : nullptr;
        }
        if (has_skip) {  // the gradient's exponent travels with it: e_dy + wscale + inc
            o.exp_in = l.edy;
            o.wscale = l.ws_dev;
            o.exp_out = pv.edy;
        }
        dy16_valid[i - 1] = !skip16 && !g0_only;
        const bool dgk = !g0_only;  // (rowconv_fwd's own rule: an operand of the input-gradient epilogues)
        const bool pooled = o.pool_dx != nullptr;  // (rowconv_fwd's own rule: the gradient goes through a pool)
        const int rc = rowconv_ranged(rowconv_fused_ok(d, dgk, pooled), rowconv_acc_bytes(d, dgk, pooled) != 0, o, rng(i, 1), l.bar,
                                      l.epoch, st,
                                      [&](const RowConvOut& ro, int mode, uint32_t* bar, uint32_t epoch, uint32_t* err) {
                                          return rowconv_fwd(d, dyin, l.wft, ro, mode, rng(i, 1), bar, epoch, err, st);
                                      });
        if (rc != NITI_NO_ERROR) return rc;
        probe(i, 1, false, st);
        dp16_valid[i - 1] = o.p16 != nullptr ? 1 : 0;
        dyc32_valid[i - 1] = next != nullptr ? 1 : 0;
        return NITI_NO_ERROR;
    }
    dy16_valid[i - 1] = 1;
    const ConvGeom& pg = pv.g;
    // (a depthwise layer: its own two launches below, the fall-back's plain outputs around them)
    // (a strided layer on its sub-pixel class GEMMs: plain outputs too -- their requantise takes no others)
    const bool sub = l.subw != nullptr;
    const bool spec = !l.dw && conv_dgrad_spec_ok(g);
    // dy of layer i - 1 is rewritten here; its P16 copy comes along where the requant pass can
    // write it (the plain and the fused pool-gradient passes), else wgrad_layer converts it
    int8_t* p16_out = !l.dw && !sub && !spec && fuse_dp16 && wgrad_p16_splits(i - 1) > 0 ? dp16[i - 1] : nullptr;
    dp16_valid[i - 1] = 0;
    // the previous layer is a skip's source: the input gradient unmasked into sum_tmp, the sum after it
    const bool src = pv.src_of >= 0;
    ActOut o;
    bool fuse = false;
    if (has_skip) {  // the gradient's exponent travels with it: e_dy + wscale + inc
        o.exp_in = l.edy;
        o.wscale = l.ws_dev;
        o.exp_out = src ? e_tmp : pv.edy;
    }
    if (src) {
        o.out = sum_tmp;
    } else if (pv.to_1x1()) {
        o.out = pv.dflat;
    } else if (pv.pool) {
        fuse = !l.dw && !sub && !spec && pg.oh % 2 == 0 && pg.ow % 2 == 0 && conv_dgrad_phase2_separate(g, slab_bytes);
        if (fuse) {  // pool gradient + relu gradient ride along the requant pass
            o.out = nullptr;
            o.pool.x = pv.r;
            o.pool.y = pv.p;
            o.pool.dx = pv.dy;
            o.pool.relu = pv.relu;
            o.pool.H = pg.oh;
            o.pool.W = pg.ow;
            o.out_p16 = p16_out;
            // the previous layer's row-kernel input gradient reads dy as C32: the same pass writes it
            // (VGG-16 conv2_2 at 112 px: no 205 MB layout launch)
            if (p16_out == nullptr && rowconv_dgrad_layer(i - 1) && !rowconv_nhwc_pref(pv.dg) && pg.cop % 32 == 0)
                o.pool.dx_c32 = pv.dyc32;
        } else {
            o.out = pv.dtmp;
        }
    } else {
        o.relu_mask = pv.relu ? pv.r : nullptr;
        o.out = pv.dy;
        if (!l.dw && conv_dgrad_phase2_separate(g, slab_bytes)) o.out_p16 = p16_out;
    }
    // (the pair: no int32 tensor while the bit width holds)
    const int rc = gemm_ranged(
        !l.dw && !dp && !capturing && !fuse && o.out_p16 == nullptr && o.out != nullptr, spec, o, rng(i, 1), l.bar, l.epoch, st,
        [&](const ActOut& ao, const FusedBar& fb) { return conv_dgrad_fused(g, l.dy, l.wT, ao, fb, st); },
        [&](const ActOut& ao, int ph) {
            int8_t* alt = conv_dgrad_spec_alt_bytes(g) <= gspec_alt_bytes ? gspec_alt : nullptr;
            return conv_dgrad_spec(g, l.dy, l.wT, rng(i, 1), ao, l.gspec + GEMM_SPEC_SLOT_WORDS, ph, st, alt);
        },
        [&](const ActOut& ao, int ph) {
            if (l.dw) return dwconv_dgrad(g, l.dy, l.w, rng(i, 1), ao, ph - 1, st);
            return ph == 1 ? conv_dgrad_phase1(g, l.dy, l.wT, acc, rng(i, 1), slab, slab_bytes, st, l.subw)
                           : conv_dgrad_phase2(g, l.dy, l.wT, acc, rng(i, 1), ao, slab_bytes, st, l.subw);
        });
    if (rc != NITI_NO_ERROR) return rc;
    probe(i, 1, false, st);
    if (src) {
        if (const int rs = skip_sum_bwd(i - 1, st)) return rs;
    } else if (pv.gpool) {  // the pooled gradient to every pixel, then the layer's relu mask
        DTRY(sum_pool_grad(pv.dflat, n, pg.oh * pg.ow, pg.cop, pv.dy, st, pv.relu ? pv.r : nullptr));
    } else if (pv.flatten) {
        const int fhw = pv.fh() * pv.fw(), ld = round_up(pg.c_out * fhw, 16);
        const int64_t elems = (int64_t)n * fhw * pg.cop;
        // (no pool, no relu: the flatten's gradient is the layer's output gradient as it stands)
        int8_t* din = pv.pool || pv.relu ? pv.dtmp : pv.dy;
        DTRY(launch_map(elems, FlattenBwd{pv.dflat, fhw, pg.c_out, pg.cop, ld, din}, st));
        if (pv.pool)
            DTRY(maxpool_relu_grad_nhwc16(pv.r, pv.p, pv.dtmp, n, pg.oh, pg.ow, pg.cop, 2, 2, 0, pv.ph, pv.pw, pv.relu,
                                          pv.dy, st));
        else if (pv.relu)
            DTRY(relu_grad_nhwc16(pv.r, pv.dtmp, elems, pv.dy, st));
    } else if (pv.pool && !fuse) {
        DTRY(maxpool_relu_grad_nhwc16(pv.r, pv.p, pv.dtmp, n, pg.oh, pg.ow, pg.cop, 2, 2, 0, pv.ph, pv.pw, pv.relu,
                                      pv.dy, st));
    }
    if (o.out_p16 != nullptr) dp16_valid[i - 1] = 1;
    dyc32_valid[i - 1] = fuse && o.pool.dx_c32 != nullptr ? 1 : 0;
    return NITI_NO_ERROR;
}

// Per-shape plan autotuning.  For every GEMM of the step (layer x {forward, weight gradient,
// input gradient}) time the layer's whole phase -- GEMM(s), split-K reduce, requantisation,
// fused / separate pool -- under each candidate plan on the caller's stream and keep the
// fastest as a plan override (niti_kernels.hpp).  Candidates: the tap-sharing weight-gradient
// kernel where it applies and 6 GEMM tile shapes, each x {store acc,
// recompute (activation GEMMs), split-K 2..64 within the tuning workspace}.  The layer phases
// are idempotent on the buffers left by the previous step, so tuning leaves the weights
// untouched; a fixed default plan (plan_gemm) is the starting point and is kept unless beaten.
int Model::autotune(hipStream_t st, int reps) {
    if (reps < 1) reps = 5;
    const int nl = (int)L.size();
    // split-K room for the candidates
    if (!ensure_slab(size_t(96) << 20, false) || !ensure_slab(size_t(96) << 20, true)) return NITI_OUT_OF_MEMORY;
    drop_graph();
    TuneTimer timer;
    if (const int rc = timer.init(st, reps)) return rc;
    tuning = true;
    int rc = NITI_NO_ERROR;
    if (hipMemsetAsync(amax, 0, amax_bytes, st) != hipSuccess) rc = NITI_NO_EXECUTION;
    // NITI_DIAG_TUNE_LOG=1 (diagnostics): every candidate's time on stderr
    const bool log = getenv("NITI_DIAG_TUNE_LOG") != nullptr;
    for (int i = 0; i < nl && rc == NITI_NO_ERROR; ++i) {
        for (int op : {PLAN_FWD, PLAN_WGRAD, PLAN_DGRAD}) {
            if (op == PLAN_DGRAD && i == 0) continue;
            if (L[i].dw) continue;  // no GEMM plan: the depthwise launches
            if (op == PLAN_FWD && rowconv_layer(i)) continue;  // no GEMM plan: the register-fed forward
            if (op == PLAN_DGRAD && rowconv_dgrad_layer(i)) continue;
            if ((op == PLAN_FWD && head_layer(i)) || (op == PLAN_DGRAD && head_dgrad_ok(i))) continue;
            if (op == PLAN_WGRAD && head_layer(i) && L[i].g.c_out <= 32 && L[i].g.cip % 32 == 0) continue;
            const ConvGeom& g = L[i].g;
            const PlanKey key = conv_plan_key(op, g);
            auto time_op = [&](float* us) {
                return timer.time(
                    [&] { return op == PLAN_FWD ? fwd_layer(i, st) : op == PLAN_WGRAD ? wgrad_layer(i, st) : dgrad_layer(i, st); },
                    us);
            };
            auto note = [&](const PlanChoice& c, float us) {
                if (log) fprintf(stderr, "tune layer %d op %d plan (%d,%d,%d,%d) %.2f us\n", i, op, c.bm, c.bn, c.splits, c.strat, us);
            };
            plan_override_clear(key);
            const size_t wsb = ws_bytes_for(op);
            PlanChoice best = conv_plan_query(op, g, op != PLAN_WGRAD, wsb);
            if (op == PLAN_WGRAD && wgrad_p16_splits(i) > 0) {
                best.bm = best.bn = PLAN_P16_TILE;
                best.splits = wgrad_p16_splits(i);
                best.strat = best.splits > 1 ? 2 : 0;
            }
            // P16 candidates are timed without their input conversion: run() converts every
            // layer's input in one launch off the step stream when the backward pass starts
            invalidate_xp16();
            if (op == PLAN_WGRAD && conv_wgrad_p16_ok(g)) {
                if (nhwc16_to_p16(L[i].in, (int64_t)g.n * g.h * g.w, g.cip, xp16[i], st) != hipSuccess) {
                    rc = NITI_NO_EXECUTION;
                    break;
                }
                xp16_valid[i] = 1;
            }
            float best_us = 0.f;
            rc = time_op(&best_us);
            note(best, best_us);
            if (op == PLAN_WGRAD && conv_wgrad_p16_ok(g)) {
                for (int sp : {1, 2, 4, 8}) {
                    if (rc != NITI_NO_ERROR) break;
                    if (conv_wgrad_p16_workspace(g, sp) > slab_w_bytes) continue;
                    PlanChoice cand;
                    cand.bm = cand.bn = PLAN_P16_TILE;
                    cand.splits = sp;
                    cand.strat = sp > 1 ? 2 : 0;
                    plan_override_set(key, cand);
                    float us = 0.f;
                    rc = time_op(&us);
                    note(cand, us);
                    if (rc == NITI_NO_ERROR && us < best_us) {
                        best_us = us;
                        best = cand;
                    }
                }
            }
            if (rc == NITI_NO_ERROR) rc = tune_gemm_tiles(op, g, wsb, time_op, note, &best, &best_us);
            plan_override_set(key, best);
            invalidate_xp16();
            if (rc != NITI_NO_ERROR) break;
        }
    }
    if (rc == NITI_NO_ERROR) rc = tune_wgrad_batch(st, timer, log);
    if (rc == NITI_NO_ERROR) rc = tune_conv0_codes(st, timer, log);
    invalidate_xp16();
    tuning = false;
    if (hipStreamSynchronize(st) != hipSuccess) rc = NITI_NO_EXECUTION;
    return rc;
}

// The P16 weight gradients as a set, with the per-layer plans settled: the per-layer sequence and
// the one-launch batch at three item sizes, each with the combine of its slabs (the launch the
// update does first).  The fastest stays as the model's choice (wgb_tuned; 0: per layer).  The item
// sizes are timed with the merged form only; the winner is then timed with its short-K layers as
// quad items (P16_QUAD_KG), and the faster of the two stays (wgb_quad; 0: no quads).  A quad
// threshold forced through niti_diag_wgrad_quad is used as it is.
int Model::tune_wgrad_batch(hipStream_t st, TuneTimer& timer, bool log) {
    if (dp() || g_wgrad_batch == 0) return NITI_NO_ERROR;
    std::vector<int> set;
    for (int i = 0; i < (int)L.size(); ++i)
        if (wgrad_p16_splits(i) > 0 && !(probe_phase == 2 && probe_layer == i)) set.push_back(i);
    if (set.size() < 2 || set.size() > (size_t)P16_MANY_MAX_JOBS) return NITI_NO_ERROR;
    // operands as the step leaves them: every input copy, and dy's copy where the last step's input
    // gradient did not write it
    if (const int rc = convert_p16_inputs(st)) return rc;
    for (int i : set)
        if (!dp16_valid[i]) {
            const ConvGeom& g = L[i].g;
            DTRY(nhwc16_to_p16(L[i].dy, (int64_t)g.n * g.oh * g.ow, g.cop, dp16[i], st));
            dp16_valid[i] = 1;
        }
    auto combine = [&]() -> int {
        SgdJob* jobs = sgd_many.data();  // (set holds distinct layers: no more jobs than sgd_many's one per layer)
        int n = 0;
        for (int i : set) {
            SgdJob& d = L[i].defer;
            if (d.slab == nullptr) continue;
            jobs[n] = d;
            jobs[n].acc = L[i].dwacc;
            jobs[n].amax = rng(i, 2);
            ++n;
            d = SgdJob{};
        }
        return sgd_combine_many(jobs, n, st) == hipSuccess ? NITI_NO_ERROR : NITI_NO_EXECUTION;
    };
    auto per_layer = [&]() -> int {
        for (int i : set) {
            Layer& l = L[i];
            const ConvGeom& g = l.g;
            const int s = wgrad_p16_splits(i);
            const bool defer = s > 1 && l.slab16 != nullptr && conv_wgrad_p16_workspace(g, s) <= l.slab16_bytes;
            L[i].defer = SgdJob{};
            DTRY(conv_wgrad_p16(g, xp16[i], dp16[i], l.dwacc, rng(i, 2), defer ? l.slab16 : slab_w,
                                defer ? l.slab16_bytes : slab_w_bytes, s, st, nullptr, nullptr, nullptr,
                                defer ? &L[i].defer : nullptr));
        }
        return combine();
    };
    auto batched = [&]() -> int {
        if (const int rc = wgrad_batch_run(true, st)) return rc;
        return combine();
    };
    float best_us = 0.f;
    int best_t = 0;
    int rc = timer.time(per_layer, &best_us);
    if (log) fprintf(stderr, "tune wgrad set: per layer %.2f us\n", best_us);
    const int q_forced = wgrad_quad_kg(-1);
    const int q_base = q_forced >= 0 ? q_forced : 0;
    for (int t : {128, 256, 512}) {
        if (rc != NITI_NO_ERROR) break;
        rc = build_wgrad_batch(t, q_base);
        if (rc != NITI_NO_ERROR || wgb_layers.empty()) break;
        float us = 0.f;
        rc = timer.time(batched, &us);
        if (log)
            fprintf(stderr, "tune wgrad set: batch t %d (%d items, longest list %d K groups) %.2f us\n", t, wgb.n_items,
                    wgb.max_list_kg, us);
        if (rc == NITI_NO_ERROR && us < best_us) {
            best_us = us;
            best_t = t;
        }
    }
    int best_q = 0;
    if (rc == NITI_NO_ERROR && best_t > 0 && q_forced < 0) {
        rc = build_wgrad_batch(best_t, P16_QUAD_KG);
        if (rc == NITI_NO_ERROR && wgb.n_quads > 0) {
            float us = 0.f;
            rc = timer.time(batched, &us);
            if (log)
                fprintf(stderr, "tune wgrad set: batch t %d quad %d (%d items, %d quads) %.2f us against %.2f us\n", best_t,
                        P16_QUAD_KG, wgb.n_items, wgb.n_quads, us, best_us);
            if (rc == NITI_NO_ERROR && us < best_us) {
                best_us = us;
                best_q = P16_QUAD_KG;
            }
        }
    }
    if (rc == NITI_NO_ERROR) {
        wgb_tuned = best_t;
        if (q_forced < 0) wgb_quad = best_q;
    }
    if (log) fprintf(stderr, "tune wgrad set: keeps %d, quad %d\n", wgb_tuned, wgrad_quad_kg(wgb_quad));
    return rc;
}

// Layer 0's weight-gradient side both ways, with the plans settled: layer 1's input gradient through
// the pool epilogue + the GEMM + its combine, against the plain input gradient + conv0_wgrad_codes +
// its combine.  The faster stays as the model's choice (c0w_tuned); a forced mode is used as it is.
int Model::tune_conv0_codes(hipStream_t st, TuneTimer& timer, bool log) {
    c0w_force = 1;
    const bool can = conv0_codes_route();
    c0w_force = -1;
    if (!can) return NITI_NO_ERROR;
    float us[2] = {0.f, 0.f};
    int rc = NITI_NO_ERROR;
    for (int way = 0; way < 2 && rc == NITI_NO_ERROR; ++way) {
        c0w_force = way;
        rc = timer.time(
            [&]() -> int {
                if (const int r = dgrad_layer(1, st)) return r;
                return wgrad_layer(0, st);
            },
            &us[way]);
    }
    c0w_force = -1;
    if (rc == NITI_NO_ERROR) c0w_tuned = us[1] < us[0];
    if (log) fprintf(stderr, "tune conv0 wgrad: expanded %.2f us, codes %.2f us, keeps %s\n", us[0], us[1], c0w_tuned ? "codes" : "expanded");
    return rc;
}

int Model::run(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st) {
    const int nl = (int)L.size();
    const bool dp = this->dp();
    SgdJob* jobs = sgd_jobs.data();
    if (nl > (int)sgd_jobs.size()) return NITI_NOT_SUPPORT;
    InStep in_step_guard(in_step);  // weight gradients inside this step may defer their combine (defer_combine)
    for (Layer& l : L) l.defer = SgdJob{};
    if (dp) {
        const int rc = ensure_comm_stream();
        if (rc != NITI_NO_ERROR) return rc;
    }
    if (!dp && !capturing && !tuning) {
        const int rc = size_wslabs();  // (plan changes: no allocation or sync inside the step)
        if (rc != NITI_NO_ERROR) return rc;
    }
    std::fill(dyc32_valid.begin(), dyc32_valid.end(), 0);
    const bool hc = head_chain_on();  // (then the head's forward runs in the chain launch below)
    {
        const int rc = forward(x_nchw, exp_in, images, hc, st);
        if (rc != NITI_NO_ERROR) return rc;
    }
    return backward(hc, labels, jobs, st);
}

int Model::forward(const int8_t* x_nchw, int exp_in, const uint8_t* images, bool skip_head, hipStream_t st) {
    const int n = batch;
    const int nl = (int)L.size();
    const bool dp = this->dp();
    invalidate_xp16();  // the forward pass rewrites every layer input
    std::fill(xc32_valid.begin(), xc32_valid.end(), 0);
    // the range words start each step at zero: zeroed by the input statistics launch (uint8
    // images), else here
    // (by kernel in an evaluation step and inside a graph capture: niti_map.hpp, fill_kernel)
    auto fill = [&](void* p, int v, size_t bytes) {
        return eval_pass || capturing ? fill_kernel(p, v, bytes, st) : hipMemsetAsync(p, v, bytes, st);
    };
    if (x_nchw != nullptr || amax_bytes % 16 != 0) DTRY(fill(amax, 0, amax_bytes));
    // the first layer's im2col copy straight from the batch where the fused pass takes the layer
    const ConvGeom& o0 = L[0].og;
    const bool fused_in = input_fused(L[0]);
    x0_nchw_valid = fused_in;
    // the first conv's range pass rides in the im2col launch (its rows are in registers there)
    Conv0Range r0;
    if (fused_in && conv0_ok(L[0].g) && !L[0].flatten && L[0].g.cop <= 64) {
        r0.w = L[0].w;
        r0.co = L[0].g.c_out;
        r0.cop = L[0].g.cop;
        r0.amax = rng(0, 0);
    }
    conv0_ranged = r0.w != nullptr;
    if (x_nchw != nullptr) {
        DTRY(fill(exp0, exp_in, 1));
        if (fused_in)
            DTRY(input_im2col(x_nchw, false, n, in_c, in_h, in_w, o0.kh, o0.kw, o0.pt, o0.pl, nullptr, 0, 0, x0n,
                              L[0].xcol, nullptr, st, r0));
        else
            DTRY(nchw_to_nhwc16(x_nchw, n, in_c, in_h * in_w, round_up(in_c, 16), x0, st));
    } else {
        // NITIInt8Train's input quantiser (MnistUtils.cpp:83-93): batch statistics (per-block
        // partials; summed and all-reduced over the ranks in exact mode), then x and its exponent
        // ascale straight into the layer-0 input
        const int64_t px = (int64_t)n * in_c * in_h * in_w;
        int ns = 0;
        DTRY(image_stats_slots(images, px, qslots, &ns, st, amax_bytes % 16 == 0 ? amax : nullptr,
                               amax_bytes % 16 == 0 ? amax_bytes : 0));
        const unsigned long long* slots = qslots;
        if ((dp && exact) || !fused_in) {
            DTRY(stats_finalize(qslots, ns, qstats, st));
            slots = qstats;
            ns = 1;
        }
        if (dp && exact) {
            DTRY(coll->allreduce(qstats, 2, COLL_SUM_U64, st));
            DTRY(coll->allreduce(qstats + 2, 2, COLL_MAX_U64, st));
        }
        const int64_t count = dp && exact ? px * world : px;
        if (fused_in)
            DTRY(input_im2col(images, true, n, in_c, in_h, in_w, o0.kh, o0.kw, o0.pt, o0.pl, slots, ns, count, x0n,
                              L[0].xcol, exp0, st, r0));
        else
            DTRY(image_quantize(images, n, in_c, in_h * in_w, round_up(in_c, 16), qstats, count, x0, exp0, true, st));
    }
    if (L[0].kp && !fused_in) DTRY(im2col32(L[0].og, x0, L[0].xcol, st));
    for (int i = 0; i < nl - (skip_head ? 1 : 0); ++i) {
        const int rc = fwd_layer(i, st);
        if (rc != NITI_NO_ERROR) return rc;
    }
    return NITI_NO_ERROR;
}

// the step's backward half: loss gradient (or the head chain), weight and input gradients, NITI_SGD
int Model::backward(bool hc, const int32_t* labels, SgdJob* jobs, hipStream_t st) {
    const int n = batch;
    const int nl = (int)L.size();
    const bool dp = this->dp();
    // weight gradients on the side stream (not inside a graph capture)
    const bool ov = overlap && !capturing && !(dp && shared_comm);  // one communicator: one stream
    bool p16_done = false;
    {
        Layer& t = L[nl - 1];
        P16Conv jobs[P16_MAX_JOBS];
        int nj = 0;
        if (hc) {
            // the head's forward, loss gradient, weight gradient and input gradient (through the
            // last pool's recorded routes, + its C32 / P16 copies) in one launch; then, on one
            // stream, every P16 input copy in one more
            const bool with_jobs = !ov && p16_input_jobs(jobs, &nj);
            if (!with_jobs) nj = 0;
            Layer& pv = L[nl - 2];
            HeadChain h;
            h.x = t.in;
            h.xld = t.g.cip;
            h.w = t.w;
            h.wT = t.wT;
            h.n = n;
            h.K = t.g.cip;
            h.c_out = t.g.c_out;
            h.cop = t.g.cop;
            h.relu = t.relu;
            h.exp_in = pv.exp;
            h.wscale = t.ws_dev;
            h.exp_out = t.exp;
            h.logits = t.r;
            h.labels = labels;
            h.dy = t.dy;
            h.dw = t.dwacc;
            h.dw_amax = rng(nl - 1, 2);
            h.code = pv.pc;
            int8_t* next = rowconv_dgrad_layer(nl - 2) && !rowconv_nhwc_pref(pv.dg) ? pv.dyc32 : nullptr;
            h.p16 = fuse_dp16 && wgrad_p16_splits(nl - 2) > 0 ? dp16[nl - 2] : nullptr;
            h.pool_dx = skip_dy16(nl - 1, next, h.p16) ? nullptr : pv.dy;
            h.pool_dx_c32 = next;
            DTRY(head_chain(h, st));
            if (with_jobs && nj > 0) {  // (a launch of its own: see niti_head.hip)
                DTRY(nhwc16_to_p16_many(jobs, nj, st));
                for (int j = 0; j < nl; ++j)
                    if (wgrad_p16_splits(j)) xp16_valid[j] = 1;
                p16_done = true;
            }
            t.r_written = true;
            dy16_valid[nl - 1] = 1;
            dy16_valid[nl - 2] = h.pool_dx != nullptr;
            dp16_valid[nl - 2] = h.p16 != nullptr ? 1 : 0;
            dyc32_valid[nl - 2] = next != nullptr ? 1 : 0;
        } else if (!ov && p16_input_jobs(jobs, &nj) && nj > 0) {
            // one stream: the loss gradient and every P16 input copy in one launch (the copies read
            // forward activations only); A/B on one box, 8 alternating 200-step runs: median step
            // 0.395 vs 0.400 ms (profiles/r03_lossp16_ab.txt)
            DTRY(loss_grad_p16(t.r, n, t.g.c_out, t.g.cop, t.exp, labels, t.dy, jobs, nj, st));
            for (int j = 0; j < nl; ++j)
                if (wgrad_p16_splits(j)) xp16_valid[j] = 1;
            p16_done = true;
        } else {
            DTRY(loss_grad(t.r, n, t.g.c_out, t.g.cop, t.exp, labels, t.dy, st));
        }
        dp16_valid[nl - 1] = 0;
    }
    if (ov) {
        const int rc = ensure_streams();
        if (rc != NITI_NO_ERROR) return rc;
    }
    hipStream_t wst = ov ? side : st;
    // single device, one stream: the P16 weight gradients wait for the last input gradient and run
    // as one launch (wgrad_batch_run below)
    const bool wbatch = !dp && !ov && !tuning && !wgb_layers.empty();
    for (int i = nl - 1; i >= 0; --i) {
        // (an event record leaves a ~6.5 us bubble before the next launch on the step stream;
        // hipStreamWriteValue64 / WaitValue64 run as blit kernels here and cost more)
        if (ov) {  // dy_i is ready on the step stream
            DTRY(hipEventRecord(ev_dy[i], st));
            DTRY(hipStreamWaitEvent(side, ev_dy[i], 0));
        }
        if (i == nl - 1 && !p16_done) {  // the forward outputs are final: every P16 input copy in one go
            const int rc = convert_p16_inputs(wst);
            if (rc != NITI_NO_ERROR) return rc;
        }
        const bool in_chain = hc && i == nl - 1;  // (the head chain launch did both)
        int rc = in_chain || (wbatch && wgrad_batched(i)) ? NITI_NO_ERROR : wgrad_layer(i, wst);
        // data parallel: a completed gradient bucket goes to the comm stream right away
        if (rc == NITI_NO_ERROR && dp && closes_bucket[i]) rc = sum_bucket(i, wst);
        if (rc == NITI_NO_ERROR && i > 0 && !in_chain) rc = dgrad_layer(i, st);
        if (rc != NITI_NO_ERROR) return rc;
        // NITI_SGD (NITI_SGD.hpp:20-54) for this layer is deferred: every layer's update runs in one
        // launch after the backward pass (the input gradients above read the old weights); the IHWO16
        // transpose feeds only the GEMM input gradient, the int8 gradient only the
        // niti_model_get tap (keep_grads); with it the combine of this layer's split-K slabs
        jobs[i] = sgd_job(i, i > 0 && !rowconv_dgrad_layer(i));
    }
    if (wbatch) {
        // dy's P16 copy where no input-gradient epilogue wrote it, all in one launch; then the batch
        P16Conv cv[P16_MAX_JOBS];
        int nc = 0;
        for (int i : wgb_layers)
            if (!dp16_valid[i]) {
                const ConvGeom& g = L[i].g;
                cv[nc++] = P16Conv{L[i].dy, (int64_t)g.n * g.oh * g.ow, g.cop, dp16[i]};
                dp16_valid[i] = 1;
            }
        static_assert(P16_MANY_MAX_JOBS <= P16_MAX_JOBS, "one conversion launch holds every member");
        if (nc > 0) DTRY(nhwc16_to_p16_many(cv, nc, st));
        const int rc = wgrad_batch_run(defer_combine(), st);
        if (rc != NITI_NO_ERROR) return rc;
        for (int i : wgb_layers)
            if (L[i].defer.slab != nullptr) jobs[i].take_combine(L[i].defer);
    }
    if (dp) {  // every bucket summed and ranged on the comm stream before the update
        DTRY(hipEventRecord(ev_grads, cst));
        DTRY(hipStreamWaitEvent(st, ev_grads, 0));
    } else if (ov) {  // every weight gradient is in before the update
        DTRY(hipEventRecord(ev_side, side));
        DTRY(hipStreamWaitEvent(st, ev_side, 0));
    }
    // the fully connected layers that took the fused form update in their own recompute pass
    SgdJob* many = sgd_many.data();
    int n_many = 0;
    for (int i = 0; i < nl; ++i)
        if (!L[i].fc_sgd) many[n_many++] = jobs[i];
    // (+ the deferred combines) also rewrites the fragment-major weight copies; one launch up to
    // SGD_MAX_JOBS layers, consecutive launches past that
    if (n_many <= SGD_MAX_JOBS) {
        DTRY(sgd_update_many(many, n_many, st, upd_bits));
    } else {
        const int rc = in_job_groups(n_many, SGD_MAX_JOBS,
                                     [&](int first, int count) { return sgd_update_many(many + first, count, st, upd_bits); });
        if (rc != NITI_NO_ERROR) return rc;
    }
    for (int i = 0; i < nl; ++i)
        if (L[i].fc_sgd) DTRY(conv_wgrad_fc_sgd(L[i].g, L[i].in, L[i].dy, rng(i, 2), jobs[i], 1, st, upd_bits));
    g8_written = keep_grads;
    return NITI_NO_ERROR;
}

// Forward-only step: the training step's forward half (the head through fwd_layer, whatever the
// head chain setting) as direct launches on `st` -- the training graph is neither dropped nor
// replayed -- then the head metrics of the logits into the running totals.  Writes the forward's
// buffers and validity flags only: no weight, derived copy, gradient or SGD state.  The armed
// kernel probe does not time evaluation launches.
int Model::eval(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st) {
    const bool paused = probe_paused;
    probe_paused = true;
    eval_pass = true;
    const int rc = forward(x_nchw, exp_in, images, false, st);
    eval_pass = false;
    probe_paused = paused;
    if (rc != NITI_NO_ERROR) return rc;
    const Layer& t = L.back();
    DTRY(head_metrics(t.r, batch, t.g.c_out, t.g.cop, t.exp, labels, std::min(ev_topk, t.g.c_out), ev_pred, nullptr,
                      ev_totals, ev_ws, ev_ws_bytes, st));
    return NITI_NO_ERROR;
}

// Every layer's weights and weight scale from `src` (same architecture and input size, any batch),
// device to device on `st`, then this model's derived copies (IHWO16, fragment-major) from them.
int Model::copy_weights_from(StepDriver& other, hipStream_t st) {
    Model* sp = dynamic_cast<Model*>(&other);
    if (sp == nullptr) return NITI_INVALID_VALUE;
    Model& src = *sp;
    if (src.arch != arch || src.in_h != in_h || src.in_w != in_w || src.in_c != in_c || src.L.size() != L.size())
        return NITI_INVALID_VALUE;
    for (size_t i = 0; i < L.size(); ++i) {
        const ConvGeom &a = L[i].g, &b = src.L[i].g;
        if (a.c_in != b.c_in || a.c_out != b.c_out || a.kh != b.kh || a.kw != b.kw || a.cip != b.cip || a.cop != b.cop ||
            L[i].kp != src.L[i].kp || L[i].relu != src.L[i].relu || L[i].pool != src.L[i].pool ||
            L[i].flatten != src.L[i].flatten || L[i].dw != src.L[i].dw || L[i].og.sh != src.L[i].og.sh ||
            L[i].gpool != src.L[i].gpool || L[i].skip != src.L[i].skip)
            return NITI_INVALID_VALUE;
    }
    if (&src == this) return NITI_NO_ERROR;
    return copy_layer_weights(src, st);
}

// One layer phase of the last step again, alone (single device: collectives off for the call).
int Model::run_phase(int layer, int phase, hipStream_t st) {
    if (!layer_ok(layer) || phase < 0 || phase > 2 || (phase == 1 && layer == 0)) return NITI_INVALID_VALUE;
    const bool t = tuning;
    tuning = false;  // keep the probe armed; collectives stay off (single-device phase)
    std::unique_ptr<Collective> c = std::move(coll), cg = std::move(coll_grad);
    const int rc = phase == 0 ? fwd_layer(layer, st) : phase == 1 ? dgrad_layer(layer, st) : wgrad_layer(layer, st);
    coll = std::move(c);
    coll_grad = std::move(cg);
    tuning = t;
    return rc;
}

int Model::plan_info(int layer, int phase, int info[4]) {
    if (!layer_ok(layer) || phase < 0 || phase > 2) return NITI_INVALID_VALUE;
    if (L[layer].dw) return NITI_NOT_SUPPORT;  // no GEMM plan
    const int op = plan_op(phase);
    PlanChoice c = conv_plan_query(op, L[layer].g, phase != 2, ws_bytes_for(op));
    if (phase == 2 && wgrad_p16_splits(layer) > 0) {
        c.bm = c.bn = PLAN_P16_TILE;
        c.splits = wgrad_p16_splits(layer);
        c.strat = c.splits > 1 ? 2 : 0;
    }
    return plan_out(c, info);
}

// this driver's own rule: the P16 tile (weight gradients the P16 kernel takes), at most 64 splits,
// over the weight-gradient slab it grows here
int Model::plan_set(int layer, int phase, const int plan[4]) {
    if (!layer_ok(layer) || phase < 0 || phase > 2) return NITI_INVALID_VALUE;
    if (L[layer].dw) return NITI_NOT_SUPPORT;  // no GEMM plan
    const int op = plan_op(phase);
    const ConvGeom& g = L[layer].g;
    const PlanKey k = conv_plan_key(op, g);
    if (plan == nullptr) {
        plan_override_clear(k);
    } else {
        const bool p16 = plan[0] == PLAN_P16_TILE && plan[1] == PLAN_P16_TILE && op == PLAN_WGRAD && conv_wgrad_p16_ok(g);
        if (!plan_valid(op, g, plan, p16)) return NITI_INVALID_VALUE;
        if (p16) {
            if (plan[2] > 64) return NITI_INVALID_VALUE;
            if (!ensure_slab(conv_wgrad_p16_workspace(g, plan[2]), true)) return NITI_OUT_OF_MEMORY;
        }
        if (const int rc = plan_commit(k, op, plan, !p16)) return rc;
    }
    drop_graph();
    return NITI_NO_ERROR;
}

int Model::probe_alloc(int phase, int max_launches) {
    if (phase == 2 && max_launches > 0) {  // per launch, a {start, end} pair per block (zero: no block)
        const size_t bytes = (size_t)max_launches * 2 * SPAN_MAX_BLOCKS * 8;
        if (hipMalloc(&span, bytes) != hipSuccess || hipMemset(span, 0, bytes) != hipSuccess) return NITI_OUT_OF_MEMORY;
        span_cap = max_launches;
    }
    return NITI_NO_ERROR;
}

int Model::probe_read_span(double* total_ms, int* count) {
    *total_ms = 0;
    *count = 0;
    if (span == nullptr || span_count == 0) return NITI_NO_ERROR;
    int dev = 0, khz = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
        return NITI_NO_EXECUTION;
    constexpr size_t per = 2 * SPAN_MAX_BLOCKS;
    std::vector<unsigned long long> h(per * (size_t)span_count);
    if (hipMemcpy(h.data(), span, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return NITI_NO_EXECUTION;
    double t = 0;
    int n = 0;
    for (int i = 0; i < span_count; ++i) {  // first block start to last block end of launch i
        unsigned long long lo = ~0ull, hi = 0;
        for (size_t b = 0; b < per; b += 2) {
            const unsigned long long s0 = h[per * i + b], s1 = h[per * i + b + 1];
            if (s1 == 0) continue;
            lo = s0 < lo ? s0 : lo;
            hi = s1 > hi ? s1 : hi;
        }
        if (hi > lo) {
            t += (double)(hi - lo) / khz;  // ticks / kHz = ms
            ++n;
        }
    }
    *total_ms = t;
    *count = n;
    // re-arm the slots for the next measurement
    if (hipMemset(span, 0, h.size() * 8) != hipSuccess) return NITI_NO_EXECUTION;
    span_count = 0;
    return NITI_NO_ERROR;
}

// ------------------------------------------------------------------------------ host access
int Model::get_input(int8_t* x_nchw_host, int* ascale, hipStream_t st) {
    const int n = batch, hw = in_h * in_w;
    if (hipStreamSynchronize(st) != hipSuccess) return NITI_NO_EXECUTION;
    const size_t need = (size_t)n * in_c * hw;
    int8_t* tmp = nullptr;
    if (hipMalloc(&tmp, need) != hipSuccess) return NITI_OUT_OF_MEMORY;
    int8_t e = 0;
    hipError_t err = x0_nchw_valid ? hipMemcpy(tmp, x0n, need, hipMemcpyDeviceToDevice)
                                   : nhwc16_to_nchw(x0, n, in_c, hw, round_up(in_c, 16), tmp, nullptr);
    if (err == hipSuccess) err = hipMemcpy(x_nchw_host, tmp, need, hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(&e, exp0, 1, hipMemcpyDeviceToHost);
    (void)hipFree(tmp);
    if (ascale) *ascale = e;
    return err == hipSuccess ? NITI_NO_ERROR : NITI_NO_EXECUTION;
}

// The debug taps: what the last step left of layer `layer` (0 its conv (+relu) output, 1 its int8
// weight gradient, 2 its output gradient), rebuilt where the step's route never wrote it in NHWC16.
int Model::get_tap(int layer, int which, int8_t* host, size_t bytes, hipStream_t st) {
    if (!layer_ok(layer)) return NITI_INVALID_VALUE;
    const Layer& l = L[layer];
    const ConvGeom& g = l.g;
    if (hipStreamSynchronize(st) != hipSuccess) return NITI_NO_EXECUTION;
    // (a pooled layer whose route went as codes under keep_grads(0))
    if (which == 0) return l.r_written ? tap_out(l, 0, l.r, host, bytes) : NITI_INVALID_VALUE;
    const bool codes = layer == 0 && dy0_codes;  // the codes route never wrote dy: rebuilt from g0 and the codes
    if (which != 2 || (!codes && dy16_valid[layer])) return tap_out(l, which, which == 2 ? l.dy : l.g8, host, bytes);
    int8_t* d16 = nullptr;  // (else from the C32 copy the step wrote)
    const int64_t elems = (int64_t)batch * g.oh * g.ow * g.cop;
    hipError_t e = hipMalloc(&d16, (size_t)elems);
    if (e == hipSuccess)
        e = codes ? launch_map(elems, ExpandPoolCodes{l.dy, l.pc, g.oh, g.ow, g.cop, d16}, nullptr)
                  : c32_to_nhwc16(l.dyc32, batch, g.oh * g.ow, g.cop, g.c_out, d16, nullptr);
    const int rc = e == hipSuccess ? tap_out(l, 2, d16, host, bytes) : NITI_NO_EXECUTION;
    if (d16) (void)hipFree(d16);
    return rc;
}

std::unique_ptr<StepDriver> make_chain_list_driver(const niti_chain_layer3* layers, int n, int in_c, int in_hw, int batch,
                                                   int* rc, int rule) {
    *rc = chain_check(layers, n, in_c, in_hw, batch, nullptr, rule);  // (nothing allocated on a refusal)
    if (*rc != NITI_NO_ERROR) return nullptr;
    auto m = std::make_unique<Model>();
    *rc = m->build_chain(NITI_ARCH_CHAIN, batch, layers, n, in_c, in_hw, rule);
    if (*rc != NITI_NO_ERROR) return nullptr;
    return m;
}

std::unique_ptr<StepDriver> make_chain_driver(int arch, int batch, int in_hw, int* rc) {
    auto m = std::make_unique<Model>();
    *rc = m->build(arch, batch, in_hw);
    if (*rc != NITI_NO_ERROR) return nullptr;
    return m;
}

}  // namespace niti
