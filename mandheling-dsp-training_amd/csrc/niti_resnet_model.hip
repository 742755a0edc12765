// niti_resnet_model.hip -- the NITI int8 training step of a residual network on the device, driven
// from C++: ResNet-18 (BASELINE config 5) or any stage list of basic blocks (niti_resnet_spec;
// declarations and the rules' provenance in niti_resnet_model.hpp).  Described for ResNet-18:
//
// One step (uint8 images or int8 x in, NITI_SGD out), every op on the step stream:
//   input      image statistics -> [SUM / MAX over ranks] -> quantise (NCHW) -> the stem's im2col
//   stem       conv1 7x7 / 2 as a 1x1 conv over its im2col (+relu), 3x3 / 2 max pool
//   blocks     conv a (+relu), conv b, [1x1 / 2 projection], the residual sum: range pass ->
//              [MAX] -> requantise + relu with the sum recomputed from the int8 operands
//   head       global sum pool -> requantise -> fc (1x1 conv) -> NITI_LOSS_Grad
//   backward   per conv the weight gradient (descending layer order, so gradient buckets close in
//              memory order) and the input gradient with the previous relu gradient fused; the
//              residual gradient sums with the next block-output relu gradient fused; the stem's
//              overlapping max-pool gradient (first max wins) with its relu gradient
//   update     one NITI_SGD launch over all 21 layers (+ the row kernels' weight copies); a deeper
//              network's in consecutive launches of at most SGD_MAX_JOBS layers
// Every forward / input-gradient conv is one of the two forms the VGG driver uses: the register-fed
// row kernels with the rescale fused (stride-1 3x3 layers, niti_rowconv.hip) or the implicit-GEMM
// range + requantise phases (strided / 1x1 / deep layers, niti_kernels.hip).  Data parallel: the
// exact protocol of niti_model.hip (ranges MAX-reduced on the step stream between the two launches
// of each requantisation, int32 weight-gradient buckets SUM-reduced on the comm stream while the
// backward pass goes on), so N ranks equal one device running the global batch bit for bit.
// An RConv is the base's ParamLayer (niti_step_driver.hpp) plus this driver's buffers; the host access
// over the convs (weights and their derived copies, taps, logits, layer_info, spec_stats) and the update
// jobs (sgd_job) are the base's, over StepDriver::P.  Here: set_weight's drop_graph() and get_tap's
// refusal of the stem output a step did not write.
#include <string.h>

#include <algorithm>
#include <array>
#include <set>

#include "../../include/niti_hip.h"
#include "niti_map.hpp"
#include "niti_resnet_model.hpp"

namespace niti {

static ConvGeom make_geom(int n, int ci, int h, int co, int k, int s, int p) {
    ConvGeom g{};
    g.n = n;
    g.c_in = ci;
    g.h = g.w = h;
    g.c_out = co;
    g.kh = g.kw = k;
    g.sh = g.sw = s;
    g.pt = g.pl = g.pb = g.pr = p;
    g.dh = g.dw = 1;
    g.finalize();
    return g;
}

// ------------------------------------------------------------------------------ the stage list
// The largest tensor of a layer (elements, at the model's batch): the GEMM loaders address int8
// operands with 31-bit byte offsets and the int32 accumulator of a tensor is four times its size.
// The stem's im2col is an int8 operand only, never an accumulator: 2^31 - 1 bytes.
constexpr int64_t RESNET_MAX_ELEMS = int64_t(1) << 29;
constexpr int64_t RESNET_SAT = int64_t(1) << 31;
// a * b, or RESNET_SAT once it reaches it (operands >= 0; no product overflows int64)
static int64_t sat_mul(int64_t a, int64_t b) {
    if (a >= RESNET_SAT || b >= RESNET_SAT) return RESNET_SAT;
    return std::min(a * b, RESNET_SAT);
}

// one derived parameter layer: {c_in, c_out, k, stride, pad, h_in, oh, relu}
using RShape = std::array<int, 8>;

// The rule of include/niti_hip.h (niti_model_resnet_check), shared by the check, the create call and
// build(): the parameter layers of a spec in parameter order.
int resnet_check(const niti_resnet_spec* sp, int in_hw, int batch, int* n_layers, int shapes[][8]) {
    if (sp == nullptr || in_hw < 1 || batch < 1) return NITI_INVALID_VALUE;
    const niti_resnet_spec& s = *sp;
    if (s.in_c < 1 || s.stem_kernel < 1 || s.stem_stride < 1 || s.stem_pad < 0 || s.stem_pad >= s.stem_kernel ||
        (s.stem_pool != 0 && s.stem_pool != 1) || s.width < 1 || s.n_stages < 1 || s.n_stages > NITI_RESNET_MAX_STAGES ||
        s.classes < 1)
        return NITI_INVALID_VALUE;
    // conv1 and fc, two convs a block, one projection per stage after the first (stage 0 keeps conv1's
    // width at stride 1; every later stage changes both)
    int64_t layers = 2 + (s.n_stages - 1);
    for (int i = 0; i < s.n_stages; ++i) {
        if (s.depths[i] < 1) return NITI_INVALID_VALUE;
        layers += 2 * (int64_t)s.depths[i];
    }
    if ((int64_t)in_hw + 2 * (int64_t)s.stem_pad < s.stem_kernel) return NITI_INVALID_VALUE;
    // ---- well formed from here
    if (s.in_c > 4 || s.classes > 2048) return NITI_NOT_SUPPORT;
    if (layers > NITI_RESNET_MAX_LAYERS) return NITI_NOT_SUPPORT;  // (before the walk over them)
    const int64_t kk = sat_mul(sat_mul(s.stem_kernel, s.stem_kernel), s.in_c);
    if (kk > 4096 - 31) return NITI_NOT_SUPPORT;  // the im2col's column pitch: one 16-byte chunk per thread
    const int64_t kp = (kk + 31) / 32 * 32;
    const int64_t b = batch;
    const int64_t oh0 = ((int64_t)in_hw + 2 * s.stem_pad - s.stem_kernel) / s.stem_stride + 1;
    // the input rows one output row of the stem reads, staged in the im2col's 16 KiB of LDS
    if (sat_mul(sat_mul(s.stem_kernel, (oh0 - 1) * s.stem_stride + s.stem_kernel), s.in_c) > 16384) return NITI_NOT_SUPPORT;
    if (sat_mul(sat_mul(sat_mul(b, s.in_c), in_hw), in_hw) > RESNET_MAX_ELEMS) return NITI_NOT_SUPPORT;
    if (sat_mul(sat_mul(sat_mul(b, oh0), oh0), kp) >= RESNET_SAT) return NITI_NOT_SUPPORT;
    std::vector<RShape> sh;
    bool fits = true;
    // every tensor of a layer in the padded layouts build() allocates (the row kernels' C32 copies;
    // the stem's input is the NCHW batch and its im2col, bounded above)
    auto add = [&](int64_t ci, int64_t co, int k, int st, int p, int64_t h, int relu) {
        const int64_t oh = (h + 2 * p - k) / st + 1;
        const int64_t ci32 = (std::min(ci, RESNET_SAT) + 31) / 32 * 32, co32 = (std::min(co, RESNET_SAT) + 31) / 32 * 32;
        if ((!sh.empty() && sat_mul(sat_mul(sat_mul(b, h), h), ci32) > RESNET_MAX_ELEMS) ||
            sat_mul(sat_mul(sat_mul(b, oh), oh), co32) > RESNET_MAX_ELEMS ||
            sat_mul(sat_mul(co32, (int64_t)k * k), ci32) > RESNET_MAX_ELEMS)
            fits = false;
        else
            sh.push_back({(int)ci, (int)co, k, st, p, (int)h, (int)oh, relu});
        return oh;
    };
    int64_t h = add(s.in_c, s.width, s.stem_kernel, s.stem_stride, s.stem_pad, in_hw, 1);
    if (s.stem_pool) h = (h + 2 - 3) / 2 + 1;
    int64_t ci = s.width;
    for (int stage = 0; stage < s.n_stages && fits; ++stage) {
        const int64_t co = sat_mul(s.width, int64_t(1) << stage);  // width << stage, saturating
        for (int blk = 0; blk < s.depths[stage] && fits; ++blk) {
            const int st = stage > 0 && blk == 0 ? 2 : 1;
            const int64_t ho = add(ci, co, 3, st, 1, h, 1);
            add(co, co, 3, 1, 1, ho, 0);
            if (st != 1 || ci != co) add(ci, co, 1, st, 0, h, 0);
            ci = co;
            h = ho;
        }
    }
    if (fits) add(ci, s.classes, 1, 1, 0, 1, 0);
    if (!fits) return NITI_NOT_SUPPORT;
    if (n_layers) *n_layers = (int)sh.size();
    if (shapes)
        for (size_t i = 0; i < sh.size(); ++i) std::copy(sh[i].begin(), sh[i].end(), shapes[i]);
    return NITI_NO_ERROR;
}

int ResNetModel::build(int batch_, int in_hw_, const niti_resnet_spec& spec_) {
    batch = batch_;
    in_hw = in_hw_;
    spec = spec_;
    for (int i = spec.n_stages; i < NITI_RESNET_MAX_STAGES; ++i) spec.depths[i] = 0;
    classes = spec.classes;
    int n_sh = 0;
    std::vector<RShape> sh(NITI_RESNET_MAX_LAYERS);
    if (const int rc = resnet_check(&spec, in_hw, batch, &n_sh, (int(*)[8])sh.data())) return rc;
    const int n = batch;
    // the parameter layers in parameter order (oracle/niti_resnet_ref.py resnet18_convs for
    // ResNet-18); every stage after the first halves the map (stride-2 convs and the 1x1 projections
    // agree on odd sizes too)
    auto add = [&](const RShape& v) {
        RConv c;
        c.og = c.g = make_geom(n, v[0], v[5], v[1], v[2], v[3], v[4]);
        c.relu = v[7];
        C.push_back(c);
        return (int)C.size() - 1;
    };
    stem_kp = stem_cols(spec);
    add(sh[0]);
    stem = C[0].og;
    C[0].g = make_geom(n, stem_kp, stem.oh, spec.width, 1, 1, 0);
    C[0].kp = stem_kp;
    const int ph = spec.stem_pool ? (stem.oh + 2 - 3) / 2 + 1 : stem.oh;  // block 0's input size
    for (int i = 1; i + 1 < n_sh;) {  // a block: conv a, conv b, [the 1x1 projection]
        RBlock b;
        b.a = add(sh[i++]);
        b.b = add(sh[i++]);
        if (i + 1 < n_sh && sh[i][2] == 1) b.p = add(sh[i++]);
        B.push_back(b);
    }
    const int fc = add(sh[n_sh - 1]);
    const int cpool = C[B.back().b].g.cop;  // the pooled channels as stored (the last stage's width, padded)
    const int nl = (int)C.size();
    // device exponents: 2 per conv, 4 per block, pool, loss gradient, input
    n_exps = 2 * nl + 4 * (int)B.size() + 3;
    exps = (int8_t*)ws.alloc(n_exps);
    if (!exps || hipMemset(exps, 0, n_exps) != hipSuccess) return NITI_OUT_OF_MEMORY;
    int ei = 0;
    auto exp_slot = [&]() { return exps + ei++; };
    exp0 = exp_slot();
    eg = exp_slot();
    ed = exp_slot();  // the loss gradient's exponent: 0, never written
    auto A8 = [&](size_t bytes) { return (int8_t*)ws.alloc(bytes); };
    // the input and the stem
    const int cop0 = C[0].g.cop;
    x0n = A8((size_t)n * spec.in_c * in_hw * in_hw);
    xcol = A8((size_t)n * stem.oh * stem.ow * stem_kp);
    if (spec.stem_pool) {
        p0 = A8((size_t)n * ph * ph * cop0);
        pool_ws = A8((size_t)n * ph * ph * cop0);
        if (!p0 || !pool_ws) return NITI_OUT_OF_MEMORY;
    }
    d0 = A8((size_t)n * stem.oh * stem.ow * cop0);
    if (!x0n || !xcol || !d0) return NITI_OUT_OF_MEMORY;
    size_t acc_elems = 0, grad_elems = 0;
    rc_err = (uint32_t*)ws.alloc(64);
    if (!rc_err || hipMemset(rc_err, 0, 64) != hipSuccess) return NITI_OUT_OF_MEMORY;
    res_bar = (uint32_t*)ws.alloc(ROWCONV_BAR_WORDS * 4);
    if (!res_bar || hipMemset(res_bar, 0, ROWCONV_BAR_WORDS * 4) != hipSuccess) return NITI_OUT_OF_MEMORY;
    res_slot = (uint32_t*)ws.alloc(2 * B.size() * RES_SPEC_SLOT_WORDS * 4);
    if (!res_slot || hipMemset(res_slot, 0, 2 * B.size() * RES_SPEC_SLOT_WORDS * 4) != hipSuccess)
        return NITI_OUT_OF_MEMORY;
    for (int i = 0; i < nl; ++i) {
        RConv& c = C[i];
        const ConvGeom& g = c.g;
        c.w = A8(c.w_elems());
        c.ws_dev = A8(16);
        c.g8 = A8(c.w_elems());
        c.y = A8((size_t)n * g.oh * g.ow * g.cop);
        c.y_exp = exp_slot();
        c.dx_exp = exp_slot();
        c.gspec = (uint32_t*)ws.alloc(2 * GEMM_SPEC_SLOT_WORDS * 4);
        if (!c.w || !c.ws_dev || !c.g8 || !c.y || !c.gspec) return NITI_OUT_OF_MEMORY;
        if (hipMemset(c.gspec, 0, 2 * GEMM_SPEC_SLOT_WORDS * 4) != hipSuccess) return NITI_NO_EXECUTION;
        if (hipMemset(c.w, 0, c.w_elems()) != hipSuccess || hipMemset(c.ws_dev, 0, 16) != hipSuccess)
            return NITI_NO_EXECUTION;
        if (i > 0) {
            c.wT = A8((size_t)g.c_in * g.kh * g.kw * g.cop);
            if (!c.wT) return NITI_OUT_OF_MEMORY;
            if (conv_dgrad_subpix_ok(g)) {  // the stride-2 input gradient's class weights
                c.subw = A8(conv_dgrad_subpix_bytes(g));
                if (!c.subw) return NITI_OUT_OF_MEMORY;
            }
        }
        grad_elems += (size_t)c.w_elems();
        acc_elems = std::max(acc_elems, (size_t)n * g.oh * g.ow * g.cop);
        acc_elems = std::max(acc_elems, (size_t)n * g.h * g.w * g.cip);
        slab_bytes = std::max(slab_bytes, conv_fwd_workspace(g));
        slab_bytes = std::max(slab_bytes, conv_dgrad_workspace(g));
        slab_w_bytes = std::max(slab_w_bytes, conv_wgrad_workspace(g));
        // grid-barrier state: the row kernels' fused launches and speculation slots, or the GEMM
        // path's fused-rescale launches (STRAT_FUSED)
        c.bar = (uint32_t*)ws.alloc(ROWCONV_BAR_WORDS * 4);
        if (!c.bar || hipMemset(c.bar, 0, ROWCONV_BAR_WORDS * 4) != hipSuccess) return NITI_OUT_OF_MEMORY;
        if (i > 0 && rowconv_ok(g)) {
            c.rc = 1;
            c.wf = A8(rowconv_wf_bytes(g.c_out, g.c_in));
            if (!c.wf) return NITI_OUT_OF_MEMORY;
            if (!rowconv_nhwc_pref(g) && !(c.xc32 = A8((size_t)n * round_up(g.c_in, 32) * g.h * g.w)))
                return NITI_OUT_OF_MEMORY;
            rc_acc_size = std::max(rc_acc_size, rowconv_acc_bytes(g, false));
            if (rowconv_dgrad_geom(g, &c.dg)) {
                c.rcd = 1;
                c.wft = A8(rowconv_wf_bytes(g.c_in, g.c_out));
                if (!c.wft) return NITI_OUT_OF_MEMORY;
                if (!rowconv_nhwc_pref(c.dg) && !(c.dyc32 = A8((size_t)n * g.oh * g.ow * round_up(g.c_out, 32))))
                    return NITI_OUT_OF_MEMORY;
                rc_acc_size = std::max(rc_acc_size, rowconv_acc_bytes(c.dg, true));
            }
        }
    }
    grad_bucket = (int32_t*)ws.alloc(grad_elems * 4);
    if (!grad_bucket) return NITI_OUT_OF_MEMORY;
    size_t off = 0;
    for (RConv& c : C) {
        c.dwacc = grad_bucket + off;
        off += (size_t)c.w_elems();
    }
    // wiring: inputs, outputs, gradients and their exponents
    C[0].in = xcol;
    C[0].in_exp = exp0;
    C[0].dy = d0;
    C[0].dy_exp = ed;  // (the stem's weight gradient reads no exponent)
    const int8_t* u = spec.stem_pool ? p0 : C[0].y;  // (no pool: the stem's relu'd output, always written)
    const int8_t* u_exp = C[0].y_exp;                // max pooling keeps the exponent
    for (size_t k = 0; k < B.size(); ++k) {
        RBlock& b = B[k];
        RConv& ca = C[b.a];
        RConv& cb = C[b.b];
        b.u = u;
        b.u_exp = u_exp;
        b.out_elems = (int64_t)n * cb.g.oh * cb.g.ow * cb.g.cop;
        b.in_elems = (int64_t)n * ca.g.h * ca.g.w * ca.g.cip;
        b.out = A8(b.out_elems);
        b.dh = A8((size_t)n * ca.g.oh * ca.g.ow * ca.g.cop);
        b.dua = A8(b.in_elems);
        b.du = A8(b.in_elems);
        if (!b.out || !b.dh || !b.dua || !b.du) return NITI_OUT_OF_MEMORY;
        if (b.p >= 0 && !(b.dus = A8(b.in_elems))) return NITI_OUT_OF_MEMORY;
        b.out_exp = exp_slot();
        b.ez = exp_slot();
        b.ezb = exp_slot();
        b.du_exp = exp_slot();
        ca.in = u;
        ca.in_exp = u_exp;
        ca.dy = b.dh;
        ca.dy_exp = cb.dx_exp;
        ca.dx = b.dua;
        cb.in = ca.y;
        cb.in_exp = ca.y_exp;
        cb.dx = b.dh;
        cb.dx_mask = ca.y;  // conv a's relu gradient rides along conv b's input gradient
        if (b.p >= 0) {
            C[b.p].in = u;
            C[b.p].in_exp = u_exp;
            C[b.p].dx = b.dus;
        }
        u = b.out;
        u_exp = b.out_exp;
    }
    // dz of block k is block k + 1's residual gradient (the block-output relu gradient fused in);
    // the last block's comes from the sum pool's gradient
    const int last = (int)B.size() - 1;
    B[last].dz = A8(B[last].out_elems);
    if (!B[last].dz) return NITI_OUT_OF_MEMORY;
    B[last].dz_exp = C[fc].dx_exp;
    for (int k = last - 1; k >= 0; --k) {
        B[k].dz = B[k + 1].du;
        B[k].dz_exp = B[k + 1].du_exp;
    }
    for (RBlock& b : B) {
        C[b.b].dy = b.dz;
        C[b.b].dy_exp = b.dz_exp;
        if (b.p >= 0) {
            C[b.p].dy = b.dz;
            C[b.p].dy_exp = b.dz_exp;
        }
    }
    gsum = (int32_t*)ws.alloc((size_t)n * cpool * 4);
    g8pool = A8((size_t)n * cpool);
    dg = A8((size_t)n * cpool);
    RConv& f = C[fc];
    f.in = g8pool;
    f.in_exp = eg;
    f.dy = A8((size_t)n * f.g.cop);
    f.dy_exp = ed;
    f.dx = dg;
    if (!gsum || !g8pool || !dg || !f.dy) return NITI_OUT_OF_MEMORY;
    if (ei > n_exps) return NITI_NO_EXECUTION;
    acc_bytes = acc_elems * 4;
    acc = (int32_t*)ws.alloc(acc_bytes);
    qstats = (unsigned long long*)ws.alloc(64);
    qslots = (unsigned long long*)ws.alloc((size_t)IMAGE_STATS_SLOTS * 4 * sizeof(unsigned long long));
    if (!acc || !qstats || !qslots) return NITI_OUT_OF_MEMORY;
    if (slab_bytes && !(slab = ws.alloc(slab_bytes))) return NITI_OUT_OF_MEMORY;
    if (slab_w_bytes && !(slab_w = ws.alloc(slab_w_bytes))) return NITI_OUT_OF_MEMORY;
    if (rc_acc_size && !(rc_acc = (int32_t*)ws.alloc(rc_acc_size))) return NITI_OUT_OF_MEMORY;
    for (int i = 0; i < nl; ++i) {  // the GEMM-path phases that may run the speculative pair
        if (!C[i].rc) gspec_alt_bytes = std::max(gspec_alt_bytes, conv_fwd_spec_alt_bytes(C[i].g));
        if (C[i].dx != nullptr && !C[i].rcd) gspec_alt_bytes = std::max(gspec_alt_bytes, conv_dgrad_spec_alt_bytes(C[i].g));
    }
    if (gspec_alt_bytes && !(gspec_alt = (int8_t*)ws.alloc(gspec_alt_bytes))) return NITI_OUT_OF_MEMORY;
    amax_bytes = (3 * C.size() + 2 * B.size() + 1) * MAX_BYTES;
    amax = (uint32_t*)ws.alloc(amax_bytes);
    if (!amax) return NITI_OUT_OF_MEMORY;
    // C has its final size: the base's view of the layers (ahead of alloc_update_bits, which counts them)
    for (int i = 0; i < nl; ++i) {
        C[i].wg_amax = rng(i, 2);
        P.push_back(&C[i]);
    }
    sgd_jobs.resize(nl);
    if (const int rc = alloc_eval()) return rc;
    if (const int rc = alloc_update_bits()) return rc;
    return hipDeviceSynchronize() == hipSuccess ? NITI_NO_ERROR : NITI_NO_EXECUTION;
}

void ResNetModel::probe(int layer, int phase, bool begin, hipStream_t st) {
    if (!probe_armed(layer, phase) || probe_count >= (int)ev0.size()) return;
    if (begin) {
        (void)hipEventRecord(ev0[probe_count], st);
    } else {
        (void)hipEventRecord(ev1[probe_count], st);
        ++probe_count;
    }
}

void ResNetModel::drop_graph() {
    if (gexec) (void)hipGraphExecDestroy(gexec);
    gexec = nullptr;
}

// ------------------------------------------------------------------------------ one conv phase
// Forward of conv i: the row kernel (fused single launch where the grid is resident and nothing
// sits between range and requantisation; else the speculative pair with the MAX between its
// launches), or the GEMM's range phase, [MAX], requantise phase.
int ResNetModel::fwd_conv(int i, hipStream_t st) {
    RConv& c = C[i];
    const ConvGeom& g = c.g;
    const bool dp = this->dp();
    probe(i, 0, true, st);
    if (rows_on(i)) {
        const bool xn = rowconv_nhwc_pref(g);
        if (!xn) DTRY(nhwc16_to_c32(c.in, g.n, g.h * g.w, g.cip, g.c_in, c.xc32, st));
        const int8_t* xin = xn ? c.in : c.xc32;
        RowConvOut o;
        o.x_nhwc = xn ? 1 : 0;
        o.out = c.y;
        o.exp_in = c.in_exp;
        o.wscale = c.ws_dev;
        o.exp_out = c.y_exp;
        o.relu = c.relu;
        const int rc = rowconv_ranged(rowconv_fused_ok(g), rowconv_acc_bytes(g, false) != 0, o, rng(i, 0), c.bar, c.epoch,
                                      st, [&](const RowConvOut& ro, int mode, uint32_t* bar, uint32_t epoch, uint32_t* err) {
                                          return rowconv_fwd(g, xin, c.wf, ro, mode, rng(i, 0), bar, epoch, err, st);
                                      });
        if (rc != NITI_NO_ERROR) return rc;
        probe(i, 0, false, st);
        return NITI_NO_ERROR;
    }
    ActOut o;
    o.out = c.y;
    o.relu = c.relu;
    o.exp_in = c.in_exp;
    o.wscale = c.ws_dev;
    o.exp_out = c.y_exp;
    if (i == 0) {  // the stem: its 3x3 / 2 max pool in the requantise pass when there is one
        stem_pooled = spec.stem_pool && !conv_fwd_spec_ok(g) && conv_fwd_phase2_separate(g, slab_bytes);
        if (stem_pooled) {
            const int ph = C[B[0].a].g.h;
            o.pool3.out = p0;
            o.pool3.arg = pool_ws;
            o.pool3.H = g.oh;
            o.pool3.W = g.ow;
            o.pool3.OH = o.pool3.OW = ph;
            if (!keep_grads) o.out = nullptr;  // (the pre-pool output: only its tap reads it)
        }
        stem_y_written = o.out != nullptr;
    }
    const int rc = gemm_ranged(
        !dp && !capturing, conv_fwd_spec_ok(g), o, rng(i, 0), c.bar, c.epoch, st,
        [&](const ActOut& ao, const FusedBar& fb) { return conv_fwd_fused(g, c.in, c.w, ao, fb, st); },
        [&](const ActOut& ao, int ph) {
            int8_t* alt = conv_fwd_spec_alt_bytes(g) <= gspec_alt_bytes ? gspec_alt : nullptr;
            return conv_fwd_spec(g, c.in, c.w, rng(i, 0), ao, c.gspec, ph, st, alt);
        },
        [&](const ActOut& ao, int ph) {
            return ph == 1 ? conv_fwd_phase1(g, c.in, c.w, acc, rng(i, 0), slab, slab_bytes, st)
                           : conv_fwd_phase2(g, c.in, c.w, acc, rng(i, 0), ao, slab_bytes, st);
        });
    if (rc != NITI_NO_ERROR) return rc;
    probe(i, 0, false, st);
    return NITI_NO_ERROR;
}

// Input gradient of conv i into c.dx (exponent dy_exp + wscale + inc), the previous op's relu
// gradient (dx_mask) fused into its requantisation.
int ResNetModel::dgrad_conv(int i, hipStream_t st) {
    RConv& c = C[i];
    const ConvGeom& g = c.g;
    if (c.dx == nullptr) return NITI_NO_ERROR;
    probe(i, 1, true, st);
    if (rows_dg_on(i)) {
        const ConvGeom& d = c.dg;
        const bool xn = rowconv_nhwc_pref(d);
        if (!xn) DTRY(nhwc16_to_c32(c.dy, g.n, g.oh * g.ow, g.cop, g.c_out, c.dyc32, st));
        const int8_t* dyin = xn ? c.dy : c.dyc32;
        RowConvOut o;
        o.x_nhwc = xn ? 1 : 0;
        o.out = c.dx;
        o.relu_mask = c.dx_mask;
        o.exp_in = c.dy_exp;
        o.wscale = c.ws_dev;
        o.exp_out = c.dx_exp;
        o.dgrad_slot = 1;
        const int rc = rowconv_ranged(rowconv_fused_ok(d, true), rowconv_acc_bytes(d, true) != 0, o, rng(i, 1), c.bar,
                                      c.epoch, st,
                                      [&](const RowConvOut& ro, int mode, uint32_t* bar, uint32_t epoch, uint32_t* err) {
                                          return rowconv_fwd(d, dyin, c.wft, ro, mode, rng(i, 1), bar, epoch, err, st);
                                      });
        if (rc != NITI_NO_ERROR) return rc;
        probe(i, 1, false, st);
        return NITI_NO_ERROR;
    }
    ActOut o;
    o.out = c.dx;
    o.relu_mask = c.dx_mask;
    o.exp_in = c.dy_exp;
    o.wscale = c.ws_dev;
    o.exp_out = c.dx_exp;
    // (the fused launch: stride 1)
    const int rc = gemm_ranged(
        !dp() && !capturing, conv_dgrad_spec_ok(g), o, rng(i, 1), c.bar, c.epoch, st,
        [&](const ActOut& ao, const FusedBar& fb) { return conv_dgrad_fused(g, c.dy, c.wT, ao, fb, st); },
        [&](const ActOut& ao, int ph) {
            int8_t* alt = conv_dgrad_spec_alt_bytes(g) <= gspec_alt_bytes ? gspec_alt : nullptr;
            return conv_dgrad_spec(g, c.dy, c.wT, rng(i, 1), ao, c.gspec + GEMM_SPEC_SLOT_WORDS, ph, st, alt);
        },
        [&](const ActOut& ao, int ph) {
            const int8_t* subw = subpix_on() ? c.subw : nullptr;  // stride 2: four sub-pixel class GEMMs
            return ph == 1 ? conv_dgrad_phase1(g, c.dy, c.wT, acc, rng(i, 1), slab, slab_bytes, st, subw)
                           : conv_dgrad_phase2(g, c.dy, c.wT, acc, rng(i, 1), ao, slab_bytes, st, subw);
        });
    if (rc != NITI_NO_ERROR) return rc;
    probe(i, 1, false, st);
    return NITI_NO_ERROR;
}

// Weight gradient of conv i (int32, and on one device its range; data parallel, the bucket SUM and
// the range follow on the comm stream)
int ResNetModel::wgrad_conv(int i, hipStream_t st) {
    probe(i, 2, true, st);
    const int rc = wgrad_gemm(i, C[i].in, C[i].dy, nullptr, st);
    if (rc != NITI_NO_ERROR) return rc;
    probe(i, 2, false, st);
    return NITI_NO_ERROR;
}

// Block k's residual sum (niti_resnet.hip) in one of the three forms of the range / rescale protocol:
// the sum is never stored, the requantise launch recomputes it from the int8 operands.
//   forward   the block's output: relu(requant(aligned y_b + shortcut))
//   backward  the gradient at the block's input: requant(aligned dx_a + shortcut gradient), the
//             previous block output's relu gradient fused (block 0: the stem's max-pool gradient
//             takes it)
int ResNetModel::residual_sum(int k, bool bwd, hipStream_t st) {
    RBlock& b = B[k];
    const bool proj = b.p >= 0;
    const int8_t* a = bwd ? b.dua : C[b.b].y;
    const int8_t* ea = bwd ? C[b.a].dx_exp : C[b.b].y_exp;
    const int8_t* s = bwd ? (proj ? b.dus : b.dz) : (proj ? C[b.p].y : b.u);
    const int8_t* es = bwd ? (proj ? C[b.p].dx_exp : b.dz_exp) : (proj ? C[b.p].y_exp : b.u_exp);
    const int64_t n = bwd ? b.in_elems : b.out_elems;
    int8_t* ez = bwd ? b.ezb : b.ez;
    int8_t* eo = bwd ? b.du_exp : b.out_exp;
    int8_t* out = bwd ? b.du : b.out;
    const int relu = bwd ? 0 : 1;
    const int8_t* mask = bwd && k > 0 ? B[k - 1].out : nullptr;
    uint32_t* amax = rng_blk(k, bwd ? 1 : 0);
    if (res_fused_on()) {  // one launch: the range through the in-kernel grid barrier
        const hipError_t e = residual_fused(a, ea, s, es, n, ez, eo, relu, out, res_bar, ++res_epoch, rc_err, st, mask);
        if (e != hipErrorNotSupported) {
            DTRY(e);
            return NITI_NO_ERROR;
        }
        --res_epoch;
    }
    // the speculative pair (one pass of the sum while its bit width holds; one slot per block and
    // direction), else the range pass and the requantise pass
    const bool spec = res_spec_on();
    uint32_t* slot = spec ? res_slot + (2 * k + (bwd ? 1 : 0)) * RES_SPEC_SLOT_WORDS : nullptr;
    if (spec)
        DTRY(residual_requant(a, ea, s, es, n, amax, ez, eo, relu, out, st, mask, 1, slot));
    else
        DTRY(residual_add(a, ea, s, es, n, nullptr, nullptr, amax, st));
    DTRY(range_max(amax, st));
    DTRY(residual_requant(a, ea, s, es, n, amax, ez, eo, relu, out, st, mask, spec ? 2 : 0, slot));
    return NITI_NO_ERROR;
}

// ------------------------------------------------------------------------------ the step
int ResNetModel::run(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st) {
    const int n = batch;
    const int nl = (int)C.size();
    const int fc = nl - 1;
    const bool dp = this->dp();
    if (dp) {
        const int rc = ensure_comm_stream();
        if (rc != NITI_NO_ERROR) return rc;
    }
    InStep in_step_guard(in_step);  // weight gradients inside this step may defer their combine
    for (RConv& c : C) c.defer = SgdJob{};
    if (!dp && !capturing && !tuning) {
        const int rc = size_wslabs();  // (plan changes: no allocation or sync inside the step)
        if (rc != NITI_NO_ERROR) return rc;
    }
    int rc = forward(x_nchw, exp_in, images, st);
    if (rc != NITI_NO_ERROR) return rc;
    // the loss gradient, then the backward pass
    const int ph = C[B[0].a].g.h;  // block 0's input size (the stem's pooled size)
    const RBlock& bl = B.back();
    const ConvGeom& gl = C[bl.b].g;
    RConv& f = C[fc];
    DTRY(loss_grad(f.y, n, classes, f.g.cop, f.y_exp, labels, f.dy, st));
    // backward: weight gradients in descending layer order (gradient buckets close in memory order)
    auto wg = [&](int i) {
        int r = wgrad_conv(i, st);
        if (r == NITI_NO_ERROR && dp && closes_bucket[i]) r = sum_bucket(i, st);
        return r;
    };
    if ((rc = dgrad_conv(fc, st)) != NITI_NO_ERROR || (rc = wg(fc)) != NITI_NO_ERROR) return rc;
    DTRY(sum_pool_grad(dg, n, gl.oh * gl.ow, gl.cop, bl.dz, st, bl.out));  // + the last block's relu gradient
    for (int k = (int)B.size() - 1; k >= 0; --k) {
        const RBlock& b = B[k];
        if (b.p >= 0 && (rc = wg(b.p)) != NITI_NO_ERROR) return rc;
        if ((rc = dgrad_conv(b.b, st)) != NITI_NO_ERROR || (rc = wg(b.b)) != NITI_NO_ERROR) return rc;
        if ((rc = dgrad_conv(b.a, st)) != NITI_NO_ERROR || (rc = wg(b.a)) != NITI_NO_ERROR) return rc;
        if (b.p >= 0 && (rc = dgrad_conv(b.p, st)) != NITI_NO_ERROR) return rc;
        if ((rc = residual_sum(k, true, st)) != NITI_NO_ERROR) return rc;
    }
    // the stem: overlapping 3x3 / 2 max-pool gradient (first max wins) with the relu gradient, then
    // its weight gradient over the im2col
    // (the relu mask from the pooled output: the pre-pool output may not exist)
    // (no pool: the relu gradient alone, the stem's relu'd output as its mask)
    if (spec.stem_pool)
        DTRY(maxpool_relu_grad_arg(nullptr, pool_ws, B[0].du, n, stem.oh, stem.ow, C[0].g.cop, 3, 2, 1, ph, ph, 1, d0, st, p0));
    else
        DTRY(relu_grad_nhwc16(C[0].y, B[0].du, (int64_t)n * stem.oh * stem.ow * C[0].g.cop, d0, st));
    if ((rc = wg(0)) != NITI_NO_ERROR) return rc;
    if (dp) {  // every bucket summed and ranged before the update
        if (!shared_comm) {
            DTRY(hipEventRecord(ev_grads, cst));
            DTRY(hipStreamWaitEvent(st, ev_grads, 0));
        }
    }
    // NITI_SGD (NITI_SGD.hpp:20-54) for every layer in one launch (more than SGD_MAX_JOBS layers: in
    // consecutive launches, each group's deferred combines ahead of its update), after every input
    // gradient read the old weights; it also rewrites the row kernels' fragment-major copies and the
    // GEMM input gradient's transposed copy
    SgdJob* jobs = sgd_jobs.data();
    for (int i = 0; i < nl; ++i) jobs[i] = sgd_job(i, i > 0 && !rows_dg_on(i));
    rc = in_job_groups(nl, SGD_MAX_JOBS, [&](int first, int count) { return sgd_update_many(jobs + first, count, st, upd_bits); });
    if (rc != NITI_NO_ERROR) return rc;
    g8_written = keep_grads;
    return NITI_NO_ERROR;
}

int ResNetModel::forward(const int8_t* x_nchw, int exp_in, const uint8_t* images, hipStream_t st) {
    const int n = batch;
    const int fc = (int)C.size() - 1;
    const bool dp = this->dp();
    // the range words start each step at zero: zeroed by the input statistics launch (uint8
    // images), else here
    // (by kernel in an evaluation step and inside a graph capture: niti_map.hpp, fill_kernel)
    const bool by_kernel = eval_pass || capturing;
    auto fill = [&](void* p, int v, size_t bytes) {
        return by_kernel ? fill_kernel(p, v, bytes, st) : hipMemsetAsync(p, v, bytes, st);
    };
    if (images == nullptr || amax_bytes % 16 != 0) DTRY(fill(amax, 0, amax_bytes));
    // input: NITIInt8Train's quantiser (MnistUtils.cpp:83-93) on uint8 images, or int8 x as given
    const int64_t px = (int64_t)n * spec.in_c * in_hw * in_hw;
    const int8_t* xq = x_nchw;
    if (images != nullptr) {
        int ns = 0;
        DTRY(image_stats_slots(images, px, qslots, &ns, st, amax_bytes % 16 == 0 ? amax : nullptr,
                               amax_bytes % 16 == 0 ? amax_bytes : 0));
        DTRY(stats_finalize(qslots, ns, qstats, st));
        if (dp && exact) {
            DTRY(coll->allreduce(qstats, 2, COLL_SUM_U64, st));
            DTRY(coll->allreduce(qstats + 2, 2, COLL_MAX_U64, st));
        }
        DTRY(image_quantize(images, n, spec.in_c, in_hw * in_hw, spec.in_c, qstats, dp && exact ? px * world : px, x0n, exp0, false, st));
        xq = x0n;
    } else {
        DTRY(fill(exp0, exp_in, 1));
        DTRY(by_kernel ? copy_kernel(x0n, x_nchw, (size_t)px, st)
                       : hipMemcpyAsync(x0n, x_nchw, (size_t)px, hipMemcpyDeviceToDevice, st));
    }
    DTRY(im2col_small(stem, xq, stem_kp, xcol, st, true));
    // forward
    int rc = fwd_conv(0, st);
    if (rc != NITI_NO_ERROR) return rc;
    const int ph = C[B[0].a].g.h;  // the stem's pooled size
    if (spec.stem_pool && !stem_pooled)  // (else fused into the stem's requantise pass, or none)
        DTRY(maxpool_nhwc16(C[0].y, n, stem.oh, stem.ow, C[0].g.cop, 3, 2, 1, p0, ph, ph, st, pool_ws));  // + first-max positions
    for (int k = 0; k < (int)B.size(); ++k) {
        const RBlock& b = B[k];
        if ((rc = fwd_conv(b.a, st)) != NITI_NO_ERROR) return rc;
        if ((rc = fwd_conv(b.b, st)) != NITI_NO_ERROR) return rc;
        if (b.p >= 0 && (rc = fwd_conv(b.p, st)) != NITI_NO_ERROR) return rc;
        if ((rc = residual_sum(k, false, st)) != NITI_NO_ERROR) return rc;
    }
    // global sum pool + requantisation, the fc head
    const RBlock& bl = B.back();
    const ConvGeom& gl = C[bl.b].g;
    DTRY(sum_pool(bl.out, n, gl.oh * gl.ow, gl.cop, gsum, rng_pool(), st));
    DTRY(range_max(rng_pool(), st));
    {
        ActRequant r;
        r.acc = gsum;
        r.rows = n;
        r.ldc = gl.cop;
        r.amax = rng_pool();
        r.exp_in = bl.out_exp;
        r.exp_out = eg;
        r.out_nhwc16 = g8pool;
        DTRY(requant_act(r, st));
    }
    return fwd_conv(fc, st);
}

// Forward-only step: the training step's forward half as direct launches on `st` (the training
// graph is neither dropped nor replayed), then the head metrics of the logits into the running
// totals.  No weight, derived copy, gradient or SGD state is written.  The armed kernel probe does
// not time evaluation launches.
int ResNetModel::eval(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) return NITI_NO_EXECUTION;
    const bool cap = cs == hipStreamCaptureStatusActive;  // the caller captures it: no fused grid barrier
    if (cap && coll != nullptr) return NITI_NOT_SUPPORT;
    const bool paused = probe_paused;
    probe_paused = true;
    capturing = cap;
    eval_pass = true;
    const int rc = forward(x_nchw, exp_in, images, st);
    eval_pass = false;
    capturing = false;
    probe_paused = paused;
    if (rc != NITI_NO_ERROR) return rc;
    const RConv& f = C.back();
    DTRY(head_metrics(f.y, batch, classes, f.g.cop, f.y_exp, labels, std::min(ev_topk, classes), ev_pred, nullptr,
                      ev_totals, ev_ws, ev_ws_bytes, st));
    return NITI_NO_ERROR;
}

// Every conv's weights and weight scale from `src` (same input size and class count, any batch),
// device to device on `st`, then this model's derived copies from them.
int ResNetModel::copy_weights_from(StepDriver& other, hipStream_t st) {
    ResNetModel* sp = dynamic_cast<ResNetModel*>(&other);
    if (sp == nullptr) return NITI_INVALID_VALUE;
    ResNetModel& src = *sp;
    // (equal stage lists: the same layers)
    if (src.in_hw != in_hw || memcmp(&src.spec, &spec, sizeof(spec)) != 0 || src.C.size() != C.size()) return NITI_INVALID_VALUE;
    for (size_t i = 0; i < C.size(); ++i)
        if (C[i].w_elems() != src.C[i].w_elems()) return NITI_INVALID_VALUE;
    if (&src == this) return NITI_NO_ERROR;
    return copy_layer_weights(src, st);
}

int ResNetModel::step(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) return NITI_NO_EXECUTION;
    if (cs == hipStreamCaptureStatusActive) {  // the caller captures the step: no fused grid barrier in it
        if (coll != nullptr) return NITI_NOT_SUPPORT;
        capturing = true;
        const int rc = run(x_nchw, exp_in, images, labels, st);
        capturing = false;
        return rc;
    }
    if (!use_graph || coll != nullptr) return run(x_nchw, exp_in, images, labels, st);
    const void* kx = x_nchw ? (const void*)x_nchw : (const void*)images;
    if (gexec == nullptr || kx != gkey_x || labels != gkey_l || exp_in != gkey_e) {
        drop_graph();
        if (const int rc = ensure_graph_stream()) return rc;
        DTRY(hipStreamBeginCapture(gstream, hipStreamCaptureModeThreadLocal));
        capturing = true;
        const int rc = run(x_nchw, exp_in, images, labels, gstream);
        capturing = false;
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamEndCapture(gstream, &g);
        if (e == hipSuccess && rc == NITI_NO_ERROR) e = hipGraphInstantiate(&gexec, g, nullptr, nullptr, 0);
        if (g) (void)hipGraphDestroy(g);
        if (rc != NITI_NO_ERROR || e != hipSuccess) {
            drop_graph();
            use_graph = false;  // direct launches for this model
            (void)hipGetLastError();
            return run(x_nchw, exp_in, images, labels, st);
        }
        gkey_x = kx;
        gkey_l = labels;
        gkey_e = exp_in;
    }
    DTRY(hipEventRecord(gin, st));
    DTRY(hipStreamWaitEvent(gstream, gin, 0));
    DTRY(hipGraphLaunch(gexec, gstream));
    DTRY(hipEventRecord(gout, gstream));
    DTRY(hipStreamWaitEvent(st, gout, 0));
    return NITI_NO_ERROR;
}

// Per-shape GEMM plan autotuning of the GEMM-path phases (as Model::autotune): every candidate
// tile / strategy / K split of each forward, input-gradient and weight-gradient GEMM, timed as the
// whole conv phase on the last step's buffers; the fastest kept as a plan override (keyed by GEMM
// shape, so convs of one shape share it).  Plans never change results.
int ResNetModel::autotune(hipStream_t st, int reps) {
    if (reps < 1) reps = 5;
    if (!ensure_slab(size_t(96) << 20, false) || !ensure_slab(size_t(96) << 20, true)) return NITI_OUT_OF_MEMORY;
    drop_graph();
    TuneTimer timer;
    if (const int rc = timer.init(st, reps)) return rc;
    tuning = true;
    int rc = NITI_NO_ERROR;
    auto run_op = [&](int i, int op) {
        if (op == PLAN_FWD && i == 0) {  // the stem with its max pool (fused into a separate requantise pass)
            int r = fwd_conv(0, st);
            if (r == NITI_NO_ERROR && spec.stem_pool && !stem_pooled &&
                maxpool_nhwc16(C[0].y, batch, stem.oh, stem.ow, C[0].g.cop, 3, 2, 1, p0, C[B[0].a].g.h, C[B[0].a].g.w, st,
                               pool_ws) != hipSuccess)
                r = NITI_NO_EXECUTION;
            return r;
        }
        return op == PLAN_FWD ? fwd_conv(i, st) : op == PLAN_WGRAD ? wgrad_conv(i, st) : dgrad_conv(i, st);
    };
    const bool log = getenv("NITI_DIAG_TUNE_LOG") != nullptr;
    std::set<PlanKey> done;
    for (int i = 0; i < (int)C.size() && rc == NITI_NO_ERROR; ++i) {
        for (int op : {PLAN_FWD, PLAN_WGRAD, PLAN_DGRAD}) {
            if (op == PLAN_FWD && rows_on(i)) continue;
            if (op == PLAN_DGRAD && (C[i].dx == nullptr || rows_dg_on(i))) continue;
            const ConvGeom& g = C[i].g;
            const PlanKey key = conv_plan_key(op, g);
            if (!done.insert(key).second) continue;
            auto time_op = [&](float* us) { return timer.time([&] { return run_op(i, op); }, us); };
            auto note = [&](const PlanChoice& c, float us) {
                if (log) fprintf(stderr, "tune conv %d op %d plan (%d,%d,%d,%d) %.2f us\n", i, op, c.bm, c.bn, c.splits, c.strat, us);
            };
            plan_override_clear(key);
            const size_t wsb = op == PLAN_WGRAD ? slab_w_bytes : slab_bytes;
            PlanChoice best = conv_plan_query(op, g, op != PLAN_WGRAD, wsb);
            float best_us = 0.f;
            rc = time_op(&best_us);
            if (rc == NITI_NO_ERROR) rc = tune_gemm_tiles(op, g, wsb, time_op, note, &best, &best_us);
            plan_override_set(key, best);
        }
    }
    tuning = false;
    if (hipStreamSynchronize(st) != hipSuccess) rc = NITI_NO_EXECUTION;
    return rc;
}

int ResNetModel::run_phase(int layer, int phase, hipStream_t st) {
    if (layer < 0 || layer >= (int)C.size() || phase < 0 || phase > 2) return NITI_INVALID_VALUE;
    if (phase == 1 && C[layer].dx == nullptr) return NITI_INVALID_VALUE;
    std::unique_ptr<Collective> c = std::move(coll), cg = std::move(coll_grad);
    const int rc = phase == 0 ? fwd_conv(layer, st) : phase == 1 ? dgrad_conv(layer, st) : wgrad_conv(layer, st);
    coll = std::move(c);
    coll_grad = std::move(cg);
    return rc;
}

// ------------------------------------------------------------------------------ host access
int ResNetModel::set_weight(int i, const int8_t* w_host, int wscale) {
    const int rc = StepDriver::set_weight(i, w_host, wscale);
    drop_graph();  // (this driver captures again after a weight change; the chain driver does not)
    return rc;
}

int ResNetModel::get_tap(int layer, int which, int8_t* host, size_t bytes, hipStream_t st) {
    if (!layer_ok(layer)) return NITI_INVALID_VALUE;
    const RConv& c = C[layer];
    if (hipStreamSynchronize(st) != hipSuccess) return NITI_NO_EXECUTION;
    if (which == 0 && layer == 0 && !stem_y_written) return NITI_INVALID_VALUE;  // (not written by the last step)
    return tap_out(c, which, which == 0 ? c.y : which == 2 ? c.dy : c.g8, host, bytes);
}

int ResNetModel::get_input(int8_t* host, int* ascale, hipStream_t st) {
    if (hipStreamSynchronize(st) != hipSuccess) return NITI_NO_EXECUTION;
    int8_t e = 0;
    if (hipMemcpy(host, x0n, (size_t)batch * spec.in_c * in_hw * in_hw, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&e, exp0, 1, hipMemcpyDeviceToHost) != hipSuccess)
        return NITI_NO_EXECUTION;
    if (ascale) *ascale = e;
    return NITI_NO_ERROR;
}

int ResNetModel::plan_info(int layer, int phase, int info[4]) {
    if (!layer_ok(layer) || phase < 0 || phase > 2) return NITI_INVALID_VALUE;
    return plan_out(conv_plan_query(plan_op(phase), C[layer].g, phase != 2, phase == 2 ? slab_w_bytes : slab_bytes), info);
}

// this driver's own rule: at most 4096 splits
int ResNetModel::plan_set(int layer, int phase, const int plan[4]) {
    if (!layer_ok(layer) || phase < 0 || phase > 2) return NITI_INVALID_VALUE;
    const int op = plan_op(phase);
    const ConvGeom& g = C[layer].g;
    const PlanKey k = conv_plan_key(op, g);
    drop_graph();
    if (plan == nullptr) {
        plan_override_clear(k);
        return NITI_NO_ERROR;
    }
    if (!plan_valid(op, g, plan, false) || plan[2] > 4096) return NITI_INVALID_VALUE;
    return plan_commit(k, op, plan, true);
}

std::unique_ptr<StepDriver> make_resnet_driver(const niti_resnet_spec* spec, int in_hw, int batch, int* rc) {
    *rc = resnet_check(spec, in_hw, batch, nullptr, nullptr);  // (nothing allocated on a refusal)
    if (*rc != NITI_NO_ERROR) return nullptr;
    auto m = std::make_unique<ResNetModel>();
    *rc = m->build(batch, in_hw, *spec);
    if (*rc != NITI_NO_ERROR) return nullptr;
    return m;
}

}  // namespace niti
