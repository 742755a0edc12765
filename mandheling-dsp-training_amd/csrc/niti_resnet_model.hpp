// niti_resnet_model.hpp -- the NITI training step of a residual network of basic blocks driven from
// C++: ResNet-18 (BASELINE config 5) or the caller's own stage list (niti_resnet_spec), behind the same niti_model_* C ABI (niti_model_capi.hip) as the LeNet / VGG driver (niti_model.hip),
// on the same base (niti_step_driver.hpp).
//
// The reference has no ResNet NITI model: its graph builder would chain NITI_Conv_Int8_Module
// instances (tools/train/source/nn/NN.cpp:1181-1207) and its residual op NITI_Eltwise_Int8 is an
// empty stub (execution-engine/source/backend/cpu/NITI_Eltwise_Int8.cpp:20-28).  The convs, relu,
// max pool, loss gradient and NITI_SGD follow the reference ops; the residual add, the global sum
// pool and the gradient exponents are this library's rules (csrc/niti_resnet.hip, restated in
// oracle/niti_resnet_ref.py).
#pragma once

#include <memory>
#include <vector>

#include "niti_step_driver.hpp"

namespace niti {

// one parameter layer (conv1, per basic block conv a / conv b / the 1x1 projection, the fc head): the
// base's ParamLayer (the stem: g a 1x1 conv over its im2col, c_in = kp = the im2col columns; og the
// 7x7 / 2, pad 3 conv) and this driver's buffers
struct RConv : ParamLayer {
    ConvGeom dg{};  // the input gradient's geometry on the row kernel (rowconv_dgrad_geom)
    uint32_t epoch = 0;
    int8_t* xc32 = nullptr;    // C32 copies where the row kernel reads C32 (not NHWC16 in place)
    int8_t* dyc32 = nullptr;
    const int8_t* in = nullptr;      // input NHWC16 (the stem: its im2col)
    const int8_t* in_exp = nullptr;
    int8_t* y = nullptr;             // output NHWC16 (relu'd where relu)
    int8_t* y_exp = nullptr;
    int8_t* dy = nullptr;            // output gradient NHWC16 (conv b and the projection share one)
    const int8_t* dy_exp = nullptr;
    int8_t* dx = nullptr;            // input gradient (null: none -- the stem)
    int8_t* dx_exp = nullptr;
    const int8_t* dx_mask = nullptr; // the previous op's relu gradient fused into the input gradient
};

struct RBlock {
    int a = 0, b = 0, p = -1;   // conv indices (p: the projection, -1 none)
    const int8_t* u = nullptr;  // block input and its exponent
    const int8_t* u_exp = nullptr;
    int8_t* out = nullptr;      // relu(requant(aligned y_b + shortcut))
    int8_t* out_exp = nullptr;
    int8_t* ez = nullptr;       // the residual sum's exponent (forward)
    int8_t* dz = nullptr;       // gradient of the block output after its relu (conv b's and proj's dy)
    int8_t* dz_exp = nullptr;
    int8_t* dh = nullptr;       // conv a's output gradient (after its relu)
    int8_t* dua = nullptr;      // conv a's input gradient
    int8_t* dus = nullptr;      // the projection's input gradient
    int8_t* du = nullptr;       // gradient at the block input (the residual sum's requantisation)
    int8_t* du_exp = nullptr;
    int8_t* ezb = nullptr;      // the backward sum's exponent
    int64_t out_elems = 0, in_elems = 0;
};

struct ResNetModel final : StepDriver {
    niti_resnet_spec spec{};      // what build() made (unused depths zero: compared as a whole)
    // the stem's im2col columns: kernel^2 * in_c, padded to whole 32-column GEMM steps (7 * 7 * 3 =
    // 147 -> 160)
    static int stem_cols(const niti_resnet_spec& s) { return round_up(s.stem_kernel * s.stem_kernel * s.in_c, 32); }
    int stem_kp = 0;
    int in_hw = 0, classes = 1000;
    std::vector<RConv> C;
    std::vector<RBlock> B;
    ConvGeom stem{};              // conv1 as defined (the im2col's geometry)
    int8_t* x0n = nullptr;        // the quantised input, NCHW int8
    int8_t* exp0 = nullptr;
    int8_t* xcol = nullptr;       // the stem's im2col [n * oh * ow][stem_kp]
    // (both null without the stem pool: block 0 then reads the stem's relu'd output itself)
    int8_t* p0 = nullptr;         // 3x3 / 2 max pool of the stem output
    int8_t* pool_ws = nullptr;    // each pool window's first-max position (the pool gradient's)
    // the stem's requantise pass also max-pooled (Pool3) this step; with keep_grads off its pre-pool
    // output is then never written (its forward tap is unavailable)
    bool stem_pooled = false;
    // what the last step wrote for the debug taps (get_tap reads this, not the current
    // keep_grads): the stem's pre-pool output
    bool stem_y_written = false;
    int8_t* d0 = nullptr;         // the stem's output gradient
    int32_t* gsum = nullptr;      // global sum pool [n][the last stage's width, padded]
    int8_t* g8pool = nullptr;     // its requantisation (the fc input)
    int8_t* eg = nullptr;
    int8_t* dg = nullptr;         // the fc head's input gradient (as gsum)
    int8_t* ed = nullptr;         // the loss gradient's exponent (0)
    int8_t* exps = nullptr;       // device int8 exponents, handed out in build()
    int n_exps = 0;
    int32_t* acc = nullptr;       // shared int32 accumulator of the GEMM paths
    size_t acc_bytes = 0;
    int8_t* gspec_alt = nullptr;  // the GEMM speculative pairs' alternates (shared)
    size_t gspec_alt_bytes = 0;
    // the residual sums' single-launch form (residual_fused, NITI_RES_FUSED=1: measured slower than
    // the two launches): one grid-barrier state for all of them (in order on the step stream)
    // the stride-2 input gradients as sub-pixel classes (NITI_SUBPIX=0: the generic masked loader)
    static bool subpix_on() {
        static const bool off = getenv("NITI_SUBPIX") && atoi(getenv("NITI_SUBPIX")) == 0;
        return !off;
    }
    uint32_t* res_bar = nullptr;
    uint32_t res_epoch = 0;
    // the residual sums' speculative pairs: one slot per block and direction (residual_requant)
    uint32_t* res_slot = nullptr;
    static bool res_spec_on() {
        static const bool off = getenv("NITI_RES_SPEC") && atoi(getenv("NITI_RES_SPEC")) == 0;
        return !off;
    }
    bool res_fused_on() const {
        static const bool on = getenv("NITI_RES_FUSED") && atoi(getenv("NITI_RES_FUSED")) == 1;
        return on && !dp() && !capturing && res_bar != nullptr;
    }
    unsigned long long* qstats = nullptr;
    unsigned long long* qslots = nullptr;
    int32_t* grad_bucket = nullptr;
    uint32_t* amax = nullptr;     // 3 ranges per conv, then 2 per block, then the pool's
    size_t amax_bytes = 0;
    uint32_t* rng(int conv, int which) { return amax + (size_t)(3 * conv + which) * MAX_WORDS; }
    uint32_t* rng_blk(int blk, int bwd) { return amax + (size_t)(3 * C.size() + 2 * blk + bwd) * MAX_WORDS; }
    uint32_t* rng_pool() { return amax + (size_t)(3 * C.size() + 2 * B.size()) * MAX_WORDS; }
    // optional hipGraph replay of the single-device step: one executable
    hipGraphExec_t gexec = nullptr;
    const void* gkey_x = nullptr;
    const void* gkey_l = nullptr;
    int gkey_e = 0;

    std::vector<SgdJob> sgd_jobs;  // the update's job table (sized in build(): no allocation in a step)

    int build(int batch_, int in_hw_, const niti_resnet_spec& spec_);
    bool rows_on(int i) const { return use_rowconv && C[i].rc; }
    bool rows_dg_on(int i) const { return use_rowconv && C[i].rcd; }
    int fwd_conv(int i, hipStream_t st);
    int dgrad_conv(int i, hipStream_t st);
    int wgrad_conv(int i, hipStream_t st);
    // block k's residual sum: its output (forward) or the gradient at its input (bwd)
    int residual_sum(int k, bool bwd, hipStream_t st);
    int run(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st);
    int step(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st) override;
    // the step's forward half (input, every conv and residual sum, the pool, the fc head)
    int forward(const int8_t* x_nchw, int exp_in, const uint8_t* images, hipStream_t st);
    int eval(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st) override;
    int copy_weights_from(StepDriver& src, hipStream_t st) override;
    int autotune(hipStream_t st, int reps) override;
    int run_phase(int layer, int phase, hipStream_t st) override;
    int plan_info(int layer, int phase, int info[4]) override;
    int plan_set(int layer, int phase, const int plan[4]) override;
    void set_overlap(bool) override {}  // one stream (the weight gradients interleave with the input gradients)
    // kernel probe: the events on the step stream around one conv phase (both launches of a
    // two-launch form)
    void probe(int layer, int phase, bool begin, hipStream_t st);
    void drop_graph() override;
    int set_weight(int i, const int8_t* w_oihw_host, int wscale) override;
    int get_tap(int layer, int which, int8_t* host, size_t bytes, hipStream_t st) override;
    void logits_view(const int8_t** logits, int* classes_out, int* ld, const int8_t** exp) const override {
        const RConv& f = C.back();
        *logits = f.y;
        *classes_out = classes;
        *ld = f.g.cop;
        *exp = f.y_exp;
    }
    int get_input(int8_t* host, int* ascale, hipStream_t st) override;
    ~ResNetModel() override { drop_graph(); }  // (the rest in ~StepDriver)
};

}  // namespace niti
