// niti_step_driver.hip -- the logic the two step drivers share (niti_step_driver.hpp).
#include "niti_step_driver.hpp"

#include <string.h>

#include "niti_map.hpp"

namespace niti {

bool StepDriver::ensure_slab(size_t bytes, bool wgrad) {
    void*& p = wgrad ? slab_w : slab;
    size_t& have = wgrad ? slab_w_bytes : slab_bytes;
    if (have >= bytes) return true;
    if (hipDeviceSynchronize() != hipSuccess) return false;
    void* s2 = ws.alloc(bytes);
    if (!s2) return false;
    p = s2;
    have = bytes;
    return true;
}

StepDriver::~StepDriver() {
    StepDriver::clear_probe();
    if (cst) (void)hipStreamSynchronize(cst);
    for (auto e : ev_bucket) (void)hipEventDestroy(e);
    if (ev_grads) (void)hipEventDestroy(ev_grads);
    if (gin) (void)hipEventDestroy(gin);
    if (gout) (void)hipEventDestroy(gout);
    if (gstream) (void)hipStreamDestroy(gstream);
    coll_grad.reset();
    coll.reset();
    if (cst) (void)hipStreamDestroy(cst);
}

// ------------------------------------------------------------------------------ weight gradient
// the plan layer i's GEMM weight gradient runs with, where it splits K into slabs a combine can sum
static bool wslab_plan(const ConvGeom& g, size_t slab_w_bytes, PlanChoice* c) {
    *c = conv_plan_query(PLAN_WGRAD, g, false, slab_w_bytes);
    return c->strat == 2 && c->splits >= 2 && c->bm != PLAN_P16_TILE;
}

bool StepDriver::ensure_wslab(int i) const {
    PlanChoice c;
    if (!wslab_plan(P[i]->g, slab_w_bytes, &c)) return false;
    return P[i]->wslab_bytes >= conv_wgrad_slab_bytes(P[i]->g, c);  // (GEMM or tap-sharing slabs)
}

int StepDriver::size_wslabs() {
    if (wslab_epoch == plan_override_epoch()) return NITI_NO_ERROR;
    bool synced = false;
    for (ParamLayer* l : P) {
        ParamLayer& s = *l;
        PlanChoice c;
        if (!wslab_plan(s.g, slab_w_bytes, &c)) continue;
        const size_t need = conv_wgrad_slab_bytes(s.g, c);
        if (s.wslab_bytes >= need) continue;
        if (!synced && hipDeviceSynchronize() != hipSuccess) return NITI_NO_EXECUTION;
        synced = true;
        void* p = ws.replace(s.wslab, need);
        s.wslab = (int32_t*)p;
        s.wslab_bytes = p ? need : 0;
        if (!p) return NITI_OUT_OF_MEMORY;
    }
    wslab_epoch = plan_override_epoch();
    return NITI_NO_ERROR;
}

int StepDriver::wgrad_gemm(int i, const int8_t* x, const int8_t* dy, hipEvent_t after_gemm, hipStream_t st) {
    ParamLayer& s = *P[i];
    const bool defer = defer_combine() && ensure_wslab(i);
    // the autotuner times a split plan of the generic GEMM with the combine it will run with in
    // the step (over the tuning workspace, right behind the GEMM), not with the reduce launch the
    // step never makes; the tap-sharing kernel's plans are timed as they were (its slabs keep their
    // reduce launch where a split has under 4096 elements)
    const bool tune_defer = tuning && in_step_combine() &&
                            conv_plan_query(PLAN_WGRAD, s.g, false, slab_w_bytes).bm != PLAN_TAPS_TILE;
    s.defer = SgdJob{};
    DTRY(conv_wgrad_acc(s.g, x, dy, s.dwacc, dp() ? nullptr : s.wg_amax, defer ? s.wslab : slab_w,
                        defer ? s.wslab_bytes : slab_w_bytes, st, after_gemm, defer || tune_defer ? &s.defer : nullptr));
    if (tune_defer && s.defer.slab != nullptr) {
        SgdJob j = s.defer;
        j.acc = s.dwacc;
        j.amax = s.wg_amax;
        s.defer = SgdJob{};
        DTRY(sgd_combine_many(&j, 1, st));
    }
    return NITI_NO_ERROR;
}

// ------------------------------------------------------------------------------ data parallel
void StepDriver::plan_buckets() {
    const int nl = (int)P.size();
    bucket_lo.assign(nl, 0);
    closes_bucket.assign(nl, 0);
    size_t acc = 0;
    int hi = nl - 1;
    for (int i = nl - 1; i >= 0; --i) {
        acc += (size_t)P[i]->w_elems() * 4;
        if (acc >= bucket_min_bytes || i == 0) {
            closes_bucket[i] = 1;
            for (int j = i; j <= hi; ++j) bucket_lo[j] = i;
            acc = 0;
            hi = i - 1;
        }
    }
}

int StepDriver::ensure_comm_stream() {
    if (cst) return NITI_NO_ERROR;
    if (hipStreamCreateWithFlags(&cst, hipStreamNonBlocking) != hipSuccess) return NITI_NO_EXECUTION;
    // cross-stream hand-offs on one device need a device-scope release only
    constexpr unsigned kFlags = hipEventDisableTiming | hipEventReleaseToDevice;
    ev_bucket.assign(P.size(), nullptr);
    for (auto& e : ev_bucket)
        if (hipEventCreateWithFlags(&e, kFlags) != hipSuccess) return NITI_NO_EXECUTION;
    if (hipEventCreateWithFlags(&ev_grads, kFlags) != hipSuccess) return NITI_NO_EXECUTION;
    plan_buckets();
    return NITI_NO_ERROR;
}

// Data parallel: the bucket of layers [lo, hi] (contiguous in the gradient bucket; the weight
// gradients run in descending layer order) is complete once layer lo's weight gradient is in on
// `wst`: the comm stream waits for it, SUMs the bucket's int32 gradients over the ranks and takes
// every layer's range of the summed gradient (NITI_RangeEstimate over the global batch,
// NITI_GradientConv_Int8.cpp:274-296), while the step stream goes on with the input-gradient chain.
int StepDriver::sum_bucket(int lo, hipStream_t wst) {
    int hi = lo;
    while (hi + 1 < (int)P.size() && bucket_lo[hi + 1] == lo) ++hi;
    size_t elems = 0;
    for (int j = lo; j <= hi; ++j) elems += (size_t)P[j]->w_elems();
    bucket_jobs.resize(hi - lo + 1);
    for (int j = lo; j <= hi; ++j) bucket_jobs[j - lo] = AbsmaxJob{P[j]->dwacc, P[j]->w_elems(), P[j]->wg_amax, 0};
    hipStream_t s = wst;  // one communicator: the SUMs stay in the step's program order
    if (!shared_comm) {   // own communicator: its own stream, overlapping the rest of the backward pass
        DTRY(hipEventRecord(ev_bucket[lo], wst));
        DTRY(hipStreamWaitEvent(cst, ev_bucket[lo], 0));
        s = cst;
    }
    DTRY(coll_grad->allreduce(P[lo]->dwacc, elems, COLL_SUM_I32, s));
    // (a narrow deep network's bucket can hold more layers than one range launch takes)
    return in_job_groups(hi - lo + 1, ABSMAX_MAX_JOBS,
                         [&](int first, int count) { return absmax_many(bucket_jobs.data() + first, count, s); });
}

void StepDriver::attach(std::unique_ptr<Collective> c, std::unique_ptr<Collective> cg, bool shared, int world_,
                        int rank_, int exact_) {
    drop_graph();
    coll = std::move(c);
    coll_grad = std::move(cg);
    shared_comm = shared;
    world = world_;
    rank = rank_;
    exact = exact_ ? 1 : 0;
}

// ------------------------------------------------------------------------------ probe
void StepDriver::clear_probe() {
    for (auto e : ev0) (void)hipEventDestroy(e);
    for (auto e : ev1) (void)hipEventDestroy(e);
    ev0.clear();
    ev1.clear();
    probe_count = 0;
    probe_layer = probe_phase = -1;
}

int StepDriver::set_probe(int layer, int phase, int max_launches) {
    clear_probe();
    if (layer < 0) return NITI_NO_ERROR;
    probe_layer = layer;
    probe_phase = phase;
    ev0.resize(max_launches);
    ev1.resize(max_launches);
    for (int i = 0; i < max_launches; ++i)
        // timing events without the system-scope cache writeback / invalidate (it delays the
        // launch after the begin marker and is not needed to read the timestamps)
        if (hipEventCreateWithFlags(&ev0[i], hipEventDisableSystemFence) != hipSuccess ||
            hipEventCreateWithFlags(&ev1[i], hipEventDisableSystemFence) != hipSuccess)
            return NITI_OUT_OF_MEMORY;
    return probe_alloc(phase, max_launches);
}

int StepDriver::probe_read(double* total_ms, int* count) {
    double t = 0;
    for (int i = 0; i < probe_count; ++i) {
        float ms = 0.f;
        if (hipEventSynchronize(ev1[i]) != hipSuccess || hipEventElapsedTime(&ms, ev0[i], ev1[i]) != hipSuccess)
            return NITI_NO_EXECUTION;
        t += ms;
    }
    *total_ms = t;
    *count = probe_count;
    probe_count = 0;
    return NITI_NO_ERROR;
}

int StepDriver::probe_read_span(double* total_ms, int* count) {
    *total_ms = 0;
    *count = 0;
    return NITI_NO_ERROR;
}

// ------------------------------------------------------------------------------ graph stream
int StepDriver::ensure_graph_stream() {
    if (gstream) return NITI_NO_ERROR;
    DTRY(hipStreamCreateWithFlags(&gstream, hipStreamNonBlocking));
    DTRY(hipEventCreateWithFlags(&gin, hipEventDisableTiming));
    DTRY(hipEventCreateWithFlags(&gout, hipEventDisableTiming));
    return NITI_NO_ERROR;
}

// ------------------------------------------------------------------------------ evaluation
int StepDriver::alloc_eval() {
    ev_ws_bytes = head_metrics_workspace(batch);
    ev_ws = ws.alloc(ev_ws_bytes);
    ev_totals = (niti_eval_totals*)ws.alloc(sizeof(niti_eval_totals));
    ev_pred = (int32_t*)ws.alloc((size_t)batch * 4);
    tm_ws = ws.alloc(ev_ws_bytes);
    tm_totals = (niti_eval_totals*)ws.alloc(sizeof(niti_eval_totals));
    if (!ev_ws || !ev_totals || !ev_pred || !tm_ws || !tm_totals) return NITI_OUT_OF_MEMORY;
    if (hipMemset(ev_totals, 0, sizeof(niti_eval_totals)) != hipSuccess ||
        hipMemset(tm_totals, 0, sizeof(niti_eval_totals)) != hipSuccess ||
        hipMemset(ev_pred, 0, (size_t)batch * 4) != hipSuccess)
        return NITI_NO_EXECUTION;
    return NITI_NO_ERROR;
}

int StepDriver::eval_reset(hipStream_t st) {
    DTRY(fill_kernel(ev_totals, 0, sizeof(niti_eval_totals), st));
    return NITI_NO_ERROR;
}

int StepDriver::eval_read(niti_eval_totals* host_out, hipStream_t st) {
    DTRY(hipStreamSynchronize(st));
    DTRY(hipMemcpy(host_out, ev_totals, sizeof(niti_eval_totals), hipMemcpyDeviceToHost));
    return NITI_NO_ERROR;
}

int StepDriver::get_predictions(int32_t* pred_host, hipStream_t st) {
    DTRY(hipStreamSynchronize(st));
    DTRY(hipMemcpy(pred_host, ev_pred, (size_t)batch * 4, hipMemcpyDeviceToHost));
    return NITI_NO_ERROR;
}

// ------------------------------------------------------------------------------ dataset steps
// Steps first_step .. first_step + n_steps - 1 of the dataset's order, each the gather of its `batch`
// entries into the staging batch (a direct launch on `st`: under set_graph(1) it sits ahead of the
// replay's fence) and then step() / eval() on the staging pointers.  Everything is refused before
// the first launch: an output size (niti_dataset_set_output; the stored size by default) or channel
// count that is not the model's input, an output size other than the stored one while the order has
// no crop windows, a slice past the order's end, a padding entry (-1) in a training slice.
int StepDriver::steps_dataset(niti_dataset& ds, int64_t first_step, int n_steps, bool train, hipStream_t st) {
    int info[12];
    if (layer_info(0, info) != NITI_NO_ERROR) return NITI_INVALID_VALUE;
    if (ds.c != info[0] || ds.oh != info[4] || ds.ow != info[5]) return NITI_INVALID_VALUE;
    if (ds.window == nullptr && (ds.oh != ds.h || ds.ow != ds.w)) return NITI_INVALID_VALUE;
    if (first_step < 0 || n_steps <= 0 || first_step > ds.len() / batch - n_steps) return NITI_INVALID_VALUE;
    const int64_t lo = first_step * batch, hi = lo + (int64_t)n_steps * batch;
    if (train && std::find(ds.index_host.begin() + lo, ds.index_host.begin() + hi, -1) != ds.index_host.begin() + hi)
        return NITI_INVALID_VALUE;
    if (st_images == nullptr) {
        uint8_t* im = (uint8_t*)ws.alloc((size_t)batch * ds.c * ds.oh * ds.ow);
        int32_t* lb = (int32_t*)ws.alloc((size_t)batch * 4);
        if (!im || !lb) return NITI_OUT_OF_MEMORY;
        st_images = im;
        st_labels = lb;
    }
    const int8_t* logits = nullptr;
    const int8_t* lexp = nullptr;
    int classes = 0, ld = 0;
    logits_view(&logits, &classes, &ld, &lexp);
    for (int64_t s = first_step; s < first_step + n_steps; ++s) {
        DTRY(ds.gather(s * batch, batch, st_images, st_labels, st));
        const int rc = train ? step(nullptr, 0, st_images, st_labels, st) : eval(nullptr, 0, st_images, st_labels, st);
        if (rc != NITI_NO_ERROR) return rc;
        if (train && tm_enabled)
            DTRY(head_metrics(logits, batch, classes, ld, lexp, st_labels, std::min(ev_topk, classes), nullptr, nullptr,
                              tm_totals, tm_ws, ev_ws_bytes, st));
    }
    return NITI_NO_ERROR;
}

int StepDriver::train_metrics_reset(hipStream_t st) {
    DTRY(fill_kernel(tm_totals, 0, sizeof(niti_eval_totals), st));
    return NITI_NO_ERROR;
}

int StepDriver::train_metrics_read(niti_eval_totals* host_out, hipStream_t st) {
    DTRY(hipStreamSynchronize(st));
    DTRY(hipMemcpy(host_out, tm_totals, sizeof(niti_eval_totals), hipMemcpyDeviceToHost));
    return NITI_NO_ERROR;
}

// ------------------------------------------------------------------------------ update bits
int StepDriver::alloc_update_bits() {
    const int nl = num_layers();
    upd_bits = (int32_t*)ws.alloc((size_t)std::max(nl, 1) * 4);
    if (!upd_bits) return NITI_OUT_OF_MEMORY;
    const std::vector<int32_t> two(nl, 2);
    DTRY(hipMemcpy(upd_bits, two.data(), (size_t)nl * 4, hipMemcpyHostToDevice));
    return NITI_NO_ERROR;
}

int StepDriver::set_update_bits(int layer, int bits, hipStream_t st) {
    const int nl = num_layers();
    if (bits < 0 || bits > 7 || layer < -1 || layer >= nl) return NITI_INVALID_VALUE;
    const std::vector<int32_t> v(layer < 0 ? nl : 1, bits);
    DTRY(update_bits_set(upd_bits, layer < 0 ? 0 : layer, (int)v.size(), v.data(), st));
    return NITI_NO_ERROR;
}

int StepDriver::get_update_bits(int32_t* bits_host, hipStream_t st) {
    DTRY(hipStreamSynchronize(st));
    DTRY(hipMemcpy(bits_host, upd_bits, (size_t)num_layers() * 4, hipMemcpyDeviceToHost));
    return NITI_NO_ERROR;
}

int StepDriver::rowconv_error() {
    uint32_t e = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&e, rc_err, 4, hipMemcpyDeviceToHost) != hipSuccess)
        return NITI_NO_EXECUTION;
    return (int)e;
}

// ------------------------------------------------------------------------------ plans
bool StepDriver::plan_valid(int op, const ConvGeom& g, const int plan[4], bool own_tile) {
    auto tile_ok = [](int t) { return t == 64 || t == 128 || t == 256; };
    const bool taps = plan[0] == PLAN_TAPS_TILE && plan[1] == PLAN_TAPS_TILE && op == PLAN_WGRAD && conv_wgrad_taps_ok(g);
    return !((!taps && !own_tile && (!tile_ok(plan[0]) || !tile_ok(plan[1]))) || plan[2] < 1 || plan[3] < 0 ||
             plan[3] > 4 || ((taps || own_tile) && plan[3] == 1) || (plan[3] >= 3 && (op == PLAN_WGRAD || plan[2] != 1)));
}

int StepDriver::plan_commit(const PlanKey& k, int op, const int plan[4], bool gemm_slab) {
    PlanChoice c;
    c.bm = plan[0];
    c.bn = plan[1];
    c.splits = plan[2];
    c.strat = plan[3];
    if (c.strat == 2 && gemm_slab &&
        !ensure_slab(std::min(plan_slab_bytes(k.M, k.N, c.splits), size_t(1) << 30), op == PLAN_WGRAD))
        return NITI_OUT_OF_MEMORY;
    plan_override_set(k, c);
    return NITI_NO_ERROR;
}

int StepDriver::plan_out(const PlanChoice& c, int info[4]) {
    info[0] = c.bm;
    info[1] = c.bn;
    info[2] = c.splits;
    info[3] = c.strat;
    return NITI_NO_ERROR;
}

// ------------------------------------------------------------------------------ the update job
SgdJob StepDriver::sgd_job(int i, bool wT_by_update) const {
    const ParamLayer& p = *P[i];
    const ConvGeom& g = p.g;
    // (a depthwise layer: the c_out = 1 form of its weight, no transposed copy)
    SgdJob j{p.dwacc, p.wg_amax, -(1 + i), p.w_co(), g.c_in, g.kh * g.kw, g.cip, p.dw ? 16 : g.cop, p.w,
             wT_by_update && !p.dw ? p.wT : nullptr, keep_grads ? p.g8 : nullptr};
    j.wf = p.rc ? p.wf : nullptr;
    j.wft = p.rcd ? p.wft : nullptr;
    if (p.subw != nullptr) {  // the stride-2 input gradient's sub-pixel class weights
        j.subw = p.subw;
        j.sub_kh = g.kh;
        j.sub_kw = g.kw;
        j.sub_pt = g.pt;
        j.sub_pl = g.pl;
    }
    // the combine of this layer's split-K slabs, in the update launch
    if (p.defer.slab != nullptr) j.take_combine(p.defer);
    return j;
}

// ------------------------------------------------------------------------------ host access
int StepDriver::layer_info(int layer, int info[12]) const {
    if (!layer_ok(layer)) return NITI_INVALID_VALUE;
    const ParamLayer& p = *P[layer];
    const ConvGeom& g = p.og;  // the layer as the network defines it
    const int v[12] = {g.c_in, g.c_out, g.kh, g.kw, g.h, g.w, g.oh, g.ow, g.pt, g.sh, p.relu, p.pool};
    memcpy(info, v, sizeof(v));
    return NITI_NO_ERROR;
}

int StepDriver::refresh_copies(ParamLayer& p, hipStream_t st) {
    const ConvGeom& g = p.g;
    if (p.wT && !p.dw) DTRY(ohwi16_to_ihwo16(p.w, g.c_out, g.c_in, g.kh * g.kw, g.cip, g.cop, p.wT, st));
    if (p.subw) DTRY(conv_dgrad_subpix_weights(g, p.wT, p.subw, st));
    if (p.rc) DTRY(weights_to_wf(p.w, g.c_out, g.c_in, g.cip, false, p.wf, st));
    if (p.rcd) DTRY(weights_to_wf(p.w, g.c_out, g.c_in, g.cip, true, p.wft, st));
    return NITI_NO_ERROR;
}

int StepDriver::set_weight(int layer, const int8_t* w_host, int wscale) {
    if (!layer_ok(layer) || !w_host) return NITI_INVALID_VALUE;
    ParamLayer& p = *P[layer];
    const ConvGeom& g = p.g;
    std::vector<int8_t> colw;
    if (p.kp) {  // upload the [co][kp] im2col weights as the 1x1 geometry's OIHW
        colw.resize((size_t)g.c_out * p.kp);
        cols_from_oihw(p.og, w_host, colw.data(), p.kp);
        w_host = colw.data();
    }
    // (a depthwise layer's [C][1][k][k] is the flat order of the c_out = 1 layer's OIHW)
    const size_t n = (size_t)p.w_co() * g.c_in * g.kh * g.kw;
    int8_t* tmp = nullptr;
    if (hipMalloc(&tmp, n) != hipSuccess) return NITI_OUT_OF_MEMORY;
    int rc = NITI_NO_ERROR;
    if (hipMemcpy(tmp, w_host, n, hipMemcpyHostToDevice) != hipSuccess ||
        oihw_to_ohwi16(tmp, p.w_co(), g.c_in, g.kh * g.kw, g.cip, p.w, nullptr) != hipSuccess ||
        hipMemset(p.ws_dev, (int)(int8_t)wscale, 1) != hipSuccess)
        rc = NITI_NO_EXECUTION;
    if (rc == NITI_NO_ERROR) rc = refresh_copies(p, nullptr);
    if (rc == NITI_NO_ERROR && hipDeviceSynchronize() != hipSuccess) rc = NITI_NO_EXECUTION;
    p.wscale = (int8_t)wscale;
    (void)hipFree(tmp);
    return rc;
}

int StepDriver::get_weight(int layer, int8_t* w_host) {
    if (!layer_ok(layer) || !w_host) return NITI_INVALID_VALUE;
    const ParamLayer& p = *P[layer];
    const ConvGeom& g = p.g;
    const size_t n = (size_t)p.w_co() * g.c_in * g.kh * g.kw;
    int8_t* tmp = nullptr;
    if (hipDeviceSynchronize() != hipSuccess || hipMalloc(&tmp, n) != hipSuccess) return NITI_OUT_OF_MEMORY;
    int rc = NITI_NO_ERROR;
    std::vector<int8_t> colw(p.kp ? n : 0);
    if (ohwi16_to_oihw(p.w, p.w_co(), g.c_in, g.kh * g.kw, g.cip, tmp, nullptr) != hipSuccess ||
        hipMemcpy(p.kp ? colw.data() : w_host, tmp, n, hipMemcpyDeviceToHost) != hipSuccess)
        rc = NITI_NO_EXECUTION;
    if (rc == NITI_NO_ERROR && p.kp) oihw_from_cols(p.og, colw.data(), w_host, p.kp);
    (void)hipFree(tmp);
    return rc;
}

int StepDriver::copy_layer_weights(const StepDriver& src, hipStream_t st) {
    for (size_t i = 0; i < P.size(); ++i) {
        ParamLayer& p = *P[i];
        const ParamLayer& s = *src.P[i];
        DTRY(copy_kernel(p.w, s.w, (size_t)p.w_elems(), st));  // (by kernel: see fill_kernel in niti_map.hpp)
        DTRY(copy_kernel(p.ws_dev, s.ws_dev, 1, st));
        p.wscale = s.wscale;
        const int rc = refresh_copies(p, st);
        if (rc != NITI_NO_ERROR) return rc;
    }
    return NITI_NO_ERROR;
}

int StepDriver::set_rowconv(bool enable) {
    if (use_rowconv && !enable) {  // the GEMM input gradients read IHWO16 copies the update skipped
        for (ParamLayer* p : P)
            if (p->rcd && refresh_copies(*p, nullptr) != NITI_NO_ERROR) return NITI_NO_EXECUTION;
        if (hipDeviceSynchronize() != hipSuccess) return NITI_NO_EXECUTION;
    }
    use_rowconv = enable;
    drop_graph();
    return NITI_NO_ERROR;
}

int StepDriver::tap_out(const ParamLayer& p, int which, const int8_t* src, int8_t* host, size_t bytes) {
    const ConvGeom& g = p.g;
    size_t need = 0;
    if (which == 0 || which == 2)
        need = (size_t)batch * g.c_out * g.oh * g.ow;
    else if (which == 1 && g8_written)
        need = (size_t)p.w_co() * g.c_in * g.kh * g.kw;
    else
        return NITI_INVALID_VALUE;
    // (an im2col layer's gradient goes out in the network's own shape)
    const size_t out_need = which == 1 && p.kp ? (size_t)p.og.c_out * p.og.c_in * p.og.kh * p.og.kw : need;
    if (bytes < out_need) return NITI_INVALID_VALUE;
    int8_t* tmp = nullptr;
    if (hipMalloc(&tmp, need) != hipSuccess) return NITI_OUT_OF_MEMORY;
    hipError_t e = which == 1 ? ohwi16_to_oihw(src, p.w_co(), g.c_in, g.kh * g.kw, g.cip, tmp, nullptr)
                              : nhwc16_to_nchw(src, batch, g.c_out, g.oh * g.ow, g.cop, tmp, nullptr);
    if (which == 1 && p.kp) {
        std::vector<int8_t> colw(need);
        if (e == hipSuccess) e = hipMemcpy(colw.data(), tmp, need, hipMemcpyDeviceToHost);
        if (e == hipSuccess) oihw_from_cols(p.og, colw.data(), host, p.kp);
    } else if (e == hipSuccess) {
        e = hipMemcpy(host, tmp, need, hipMemcpyDeviceToHost);
    }
    (void)hipFree(tmp);
    return e == hipSuccess ? NITI_NO_ERROR : NITI_NO_EXECUTION;
}

int StepDriver::get_logits(int8_t* host, int* exp_out, hipStream_t st) {
    const int8_t* logits = nullptr;
    const int8_t* lexp = nullptr;
    int classes = 0, ld = 0;
    logits_view(&logits, &classes, &ld, &lexp);
    if (hipStreamSynchronize(st) != hipSuccess) return NITI_NO_EXECUTION;
    std::vector<int8_t> buf((size_t)batch * ld);
    int8_t e = 0;
    if (hipMemcpy(buf.data(), logits, buf.size(), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&e, lexp, 1, hipMemcpyDeviceToHost) != hipSuccess)
        return NITI_NO_EXECUTION;
    for (int i = 0; i < batch; ++i) memcpy(host + (size_t)i * classes, buf.data() + (size_t)i * ld, classes);
    if (exp_out) *exp_out = e;
    return NITI_NO_ERROR;
}

int64_t StepDriver::step_macs() const {
    int64_t s = 0;
    for (size_t i = 0; i < P.size(); ++i) s += P[i]->macs() * (i > 0 ? 3 : 2);
    return s;
}

int StepDriver::spec_stats(uint32_t* out, int max_layers) {
    const int nl = std::min(max_layers, (int)P.size());
    std::fill(out, out + (size_t)nl * 6, 0u);
    for (int i = 0; i < nl; ++i) {
        const ParamLayer& p = *P[i];
        for (int d = 0; d < 2; ++d) {  // forward / input-gradient slot: hint, redone launches, stored pairs
            uint32_t w[5] = {0, 0, 0, 0, 0}, gw[4] = {0, 0, 0, 0};
            if (p.bar != nullptr &&
                hipMemcpy(w, rowconv_spec_slot(p.bar, d != 0), sizeof(w), hipMemcpyDeviceToHost) != hipSuccess)
                return NITI_INVALID_VALUE;
            // the GEMM path's pair (plan strategy 3): its own slot, no store mode
            if (p.gspec != nullptr &&
                hipMemcpy(gw, p.gspec + d * GEMM_SPEC_SLOT_WORDS, sizeof(gw), hipMemcpyDeviceToHost) != hipSuccess)
                return NITI_INVALID_VALUE;
            out[i * 6 + d * 3] = std::max(w[0], gw[0]);
            out[i * 6 + d * 3 + 1] = w[2] + gw[2];
            out[i * 6 + d * 3 + 2] = w[4] + gw[3];  // the GEMM pair: misses settled from an alternate
        }
    }
    return NITI_NO_ERROR;
}

int StepDriver::spec_state(int layer, uint32_t** bar) {
    if (!layer_ok(layer)) return NITI_INVALID_VALUE;
    *bar = P[layer]->bar;
    return NITI_NO_ERROR;
}

// ------------------------------------------------------------------------------ host helpers
void cols_from_oihw(const ConvGeom& o, const int8_t* w, int8_t* wc, int kp) {
    memset(wc, 0, (size_t)o.c_out * kp);
    for (int co = 0; co < o.c_out; ++co)
        for (int c = 0; c < o.c_in; ++c)
            for (int t = 0; t < o.kh * o.kw; ++t)
                wc[(size_t)co * kp + t * o.c_in + c] = w[((size_t)co * o.c_in + c) * o.kh * o.kw + t];
}
void oihw_from_cols(const ConvGeom& o, const int8_t* wc, int8_t* w, int kp) {
    for (int co = 0; co < o.c_out; ++co)
        for (int c = 0; c < o.c_in; ++c)
            for (int t = 0; t < o.kh * o.kw; ++t)
                w[((size_t)co * o.c_in + c) * o.kh * o.kw + t] = wc[(size_t)co * kp + t * o.c_in + c];
}

}  // namespace niti
