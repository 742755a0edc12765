// niti_step_driver.hpp -- what the two whole-step training drivers behind the niti_model_* C ABI
// share: the chain driver (LeNet / VGG, niti_model.hip) and the residual driver (ResNet-18 and the
// stage lists, niti_resnet_model.hip).
//
// ParamLayer is one parameter layer as the base reads it: its geometry, its weight and the copies
// derived from it, its weight gradient with the range word, the split-K slabs and the deferred
// combine.  The drivers' own layer records (Layer, RConv) derive from it and add their activation and
// gradient buffers; each build() lists them once in StepDriver::P.
//
// StepDriver holds the state and the logic both have in the same form -- split-K slabs, the
// data-parallel gradient buckets, the range / rescale launch protocol (range_max, rowconv_ranged,
// gemm_ranged), the GEMM weight gradient with its deferred combine, a layer's NITI_SGD job (sgd_job),
// the event probe, the evaluation totals, the device-resident dataset steps, the graph stream and its
// fences, the teardown, and the host-access half of the C ABI over P: layer_info, set_weight /
// get_weight with the derived copies (refresh_copies), the copy loop of copy_weights_from,
// set_rowconv, the tap conversions (tap_out), get_logits, step_macs, spec_stats -- and declares, as
// virtuals, what else the C ABI (niti_model_capi.hip) asks of a driver.  A virtual is called at most
// once per ABI call; nothing inside a step (run(), forward(), backward(), the per-layer functions) goes
// through one: P is a plain vector.  The base does not know which driver it serves: where the two
// differ, the difference is the derived class's.
#pragma once

#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "niti_coll.hpp"
#include "niti_internal.hpp"
#include "niti_kernels.hpp"

#define DTRY(expr)                                          \
    do {                                                    \
        if ((expr) != hipSuccess) return NITI_NO_EXECUTION; \
    } while (0)

namespace niti {

// one parameter layer as the base sees it (Layer and RConv derive from it; filled by the driver's
// build()): exactly what the shared code reads
struct ParamLayer {
    ConvGeom g{};   // the layer's conv as it runs (an im2col layer: the 1x1 conv over its columns)
    ConvGeom og{};  // as the network defines it (reported; weights and taps converted to / from it)
    int relu = 0;   // relu fused into the forward requantisation
    int pool = 0;   // a 2x2 max pool behind it (chain driver)
    // a depthwise conv (chain driver; niti_depthwise.hip): g.c_out == g.c_in == C; w, dwacc, g8 and the
    // slabs are [k * k][cip], the OHWI16 form of a c_out = 1, c_in = C layer (w_co), [C][1][k][k] on
    // the host, and there is no wT
    int dw = 0;
    int kp = 0;  // the im2col column pitch of a first layer that runs over its im2col (0: not one)
    int8_t wscale = 0;
    int8_t* w = nullptr;       // OHWI16
    int8_t* ws_dev = nullptr;  // wscale, device
    // the copies derived from w (null: none), kept in step by the update launch and by refresh_copies
    int8_t* wT = nullptr;    // IHWO16 (GEMM input gradient)
    int8_t* subw = nullptr;  // stride 2: the sub-pixel classes' weights (conv_dgrad_subpix_bytes)
    int8_t* wf = nullptr;    // fragment-major (row kernels, niti_rowconv.hip): forward, input gradient
    int8_t* wft = nullptr;
    int rc = 0;   // forward on the register-fed row kernels with the fused rescale
    int rcd = 0;  // its input gradient on the same kernel
    int8_t* g8 = nullptr;       // int8 weight gradient OHWI16 (keep_grads)
    uint32_t* bar = nullptr;    // row-kernel state: grid barrier words + speculation slots
    uint32_t* gspec = nullptr;  // the GEMM path's speculative pair: forward / input-gradient hint slots
    int32_t* dwacc = nullptr;   // int32 weight gradient [w_co][kk][cip], in the contiguous gradient bucket
    uint32_t* wg_amax = nullptr;  // its range word (the driver's rng(layer, 2))
    // single device: a split-K GEMM weight gradient's own slabs (sized for the current plans at the
    // head of run(), size_wslabs), and this step's combine deferred to the NITI_SGD launch
    // (sgd_update_many; slab == null: none -- the chain driver's P16 weight gradients leave theirs
    // here too)
    int32_t* wslab = nullptr;
    size_t wslab_bytes = 0;
    SgdJob defer{};
    int w_co() const { return dw ? 1 : g.c_out; }  // output channels as the weight layouts count them
    int64_t w_elems() const { return (int64_t)w_co() * g.kh * g.kw * g.cip; }
    int64_t macs() const { return (int64_t)og.n * og.oh * og.ow * og.c_out * (dw ? 1 : og.c_in) * og.kh * og.kw; }
};

struct StepDriver {
    Workspace ws;  // (first: device memory goes last, after everything below is torn down)
    int batch = 0;
    void* slab = nullptr;    // split-K slabs of the forward / input-gradient GEMMs (step stream)
    size_t slab_bytes = 0;
    void* slab_w = nullptr;  // split-K slabs of the weight-gradient GEMMs (their own stream)
    size_t slab_w_bytes = 0;
    // grow a split-K workspace (the old one stays owned by ws until the model is destroyed)
    bool ensure_slab(size_t bytes, bool wgrad);
    uint32_t* rc_err = nullptr;  // set by an in-kernel grid barrier that timed out
    bool keep_grads = true;      // the int8 weight gradient of the last step kept for get_tap (which = 1)
    bool g8_written = false;     // the last step stored the int8 weight gradients (get_tap reads this, not keep_grads)
    bool use_rowconv = true;     // the register-fed kernels (niti_rowconv.hip) for the layers they take
    bool tuning = false;         // autotune in progress: no collectives, no probe
    bool capturing = false;
    bool in_step = false;        // run(): weight gradients may defer their combine to the update launch
    struct InStep {              // run()'s guard over in_step
        bool& f;
        explicit InStep(bool& x) : f(x) { f = true; }
        ~InStep() { f = false; }
    };
    // data parallel (niti_coll.hpp, "collectives"): ranges on the step stream through `coll`,
    // gradient-bucket SUMs on the comm stream `cst` through `coll_grad`.  Attached at any world
    // size (a world of 1 runs every collective call site on one GPU).
    std::unique_ptr<Collective> coll, coll_grad;
    int world = 1, rank = 0, exact = 1;
    bool dp() const { return coll != nullptr && coll_grad != nullptr && !tuning; }
    hipStream_t cst = nullptr;
    // the gradient SUMs share the range communicator (ncclCommSplit unavailable): they then run on
    // the weight-gradient stream itself, keeping that one communicator in program order
    bool shared_comm = false;
    std::vector<ParamLayer*> P;  // the parameter layers in layer order (build(), once its layer list is final)
    std::vector<hipEvent_t> ev_bucket;  // per layer: the bucket closed after this layer's weight gradient
    hipEvent_t ev_grads = nullptr;      // every bucket summed and ranged (the NITI_SGD join)
    size_t bucket_min_bytes = grad_bucket_bytes();
    // the bucket a layer's gradient SUM rides in: layers (backward order) accumulate until the
    // bucket holds bucket_min_bytes; closes_bucket[i] marks the layer whose weight gradient
    // completes one (its first layer in memory order is bucket_lo[i])
    std::vector<int> bucket_lo;
    std::vector<char> closes_bucket;
    void plan_buckets();
    // A job table of any length through a launch that takes at most max_jobs of them (the tables
    // travel as kernel arguments: sgd_update_many's SGD_MAX_JOBS, absmax_many's ABSMAX_MAX_JOBS):
    // launch(first, count) over consecutive groups, in order, on the caller's stream.  n <= max_jobs
    // is the one launch it always was.
    template <class Launch>
    static int in_job_groups(int n, int max_jobs, Launch&& launch) {
        for (int lo = 0; lo < n; lo += max_jobs) DTRY(launch(lo, std::min(max_jobs, n - lo)));
        return NITI_NO_ERROR;
    }
    std::vector<AbsmaxJob> bucket_jobs;  // sum_bucket's table (kept: no allocation once it has grown)
    int ensure_comm_stream();
    int sum_bucket(int lo, hipStream_t wst);
    void attach(std::unique_ptr<Collective> c, std::unique_ptr<Collective> cg, bool shared, int world_, int rank_,
                int exact_);

    // ---- the range / rescale launch protocol.  An int8 output needs its whole tensor's range before
    // it is written, so every conv phase and residual sum of a step takes one of three forms: fused
    // (one launch, the range through an in-kernel grid barrier: single device, outside a capture,
    // where the kernel says its grid is resident), the speculative pair (launch A, [MAX], launch B)
    // or range launch, [MAX], requantise launch.  The choice is made here, once; the callables are
    // the site's own kernel calls (template parameters: inlined, nothing on the heap).
    // [MAX]: one range estimate all-reduced over the ranks (exact data parallelism)
    hipError_t range_max(uint32_t* amax, hipStream_t st) {
        return dp() && exact ? coll->allreduce(amax, MAX_WORDS, COLL_MAX_U32, st) : hipSuccess;
    }
    // A row kernel (niti_rowconv.hip).  fused_ok: the site's rowconv_fused_ok / rowconv_fc_ok; stores:
    // its two-launch forms keep their accumulators in rc_acc (rowconv_acc_bytes != 0; never the
    // head); launch(o, mode, bar, epoch, err) is its rowconv_fwd / rowconv_fc call.  The pair runs on
    // `bar` (its speculation slots); the plain form passes none, which is how the kernels tell them
    // apart.
    int32_t* rc_acc = nullptr;  // the row kernels' accumulator store (two-launch store mode)
    size_t rc_acc_size = 0;
    template <class Launch>
    int rowconv_ranged(bool fused_ok, bool stores, RowConvOut& o, uint32_t* amax, uint32_t* bar, uint32_t& epoch,
                       hipStream_t st, Launch&& launch) {
        if (!dp() && !capturing && fused_ok) {
            DTRY(launch(o, 0, bar, ++epoch, rc_err));
            return NITI_NO_ERROR;
        }
        if (stores) o.acc_store = rc_acc;  // (else the second launch recomputes)
        const bool pair = rowconv_spec2_on();  // one GEMM pass while the bit width holds
        uint32_t* b = pair ? bar : nullptr;
        DTRY(launch(o, pair ? RC_SPEC_A : 1, b, 0, nullptr));
        DTRY(range_max(amax, st));
        DTRY(launch(o, pair ? RC_SPEC_B : 2, b, 0, nullptr));
        return NITI_NO_ERROR;
    }
    // An implicit GEMM (niti_kernels.hip).  allow_fused: the site's own gate for the fused launch
    // (plan strategy 4), which may still decline with hipErrorNotSupported -- its barrier epoch
    // counts only the launches made; spec: the site's conv_*_spec_ok (plan strategy 3).
    // fused(o, FusedBar), pair(o, 0 | 1) and phase(o, 1 | 2) are the site's conv_* calls.
    template <class Fused, class Pair, class Phase>
    int gemm_ranged(bool allow_fused, bool spec, const ActOut& o, uint32_t* amax, uint32_t* bar, uint32_t& epoch,
                    hipStream_t st, Fused&& fused, Pair&& pair, Phase&& phase) {
        if (allow_fused) {
            const hipError_t e = fused(o, FusedBar{bar, epoch + 1, rc_err});
            if (e != hipErrorNotSupported) {
                ++epoch;
                DTRY(e);
                return NITI_NO_ERROR;
            }
        }
        DTRY(spec ? pair(o, 0) : phase(o, 1));
        DTRY(range_max(amax, st));
        DTRY(spec ? pair(o, 1) : phase(o, 2));
        return NITI_NO_ERROR;
    }

    // ---- the GEMM-path weight gradient.  Single device, inside run(): a split-K plan leaves its
    // slabs (the layer's own, ParamLayer::wslab) to the NITI_SGD launch's combine, which sums them and
    // takes the range -- no reduce launch, no int32 round trip (NITI_DIAG_SGD_COMBINE=0: off)
    static bool sgd_combine_on() {
        static const bool off = getenv("NITI_DIAG_SGD_COMBINE") && atoi(getenv("NITI_DIAG_SGD_COMBINE")) == 0;
        return !off;
    }
    bool defer_combine() const { return in_step && sgd_combine_on() && !dp() && !capturing && !tuning; }
    // whether a step of this model defers its combines at all (what the autotuner times against)
    bool in_step_combine() const { return sgd_combine_on() && !dp(); }
    // layer i's own slab buffer is big enough for the plan it runs with (false: its plan does not
    // split K into C-shaped slabs, or the buffer was not sized)
    bool ensure_wslab(int i) const;
    // size every layer's slab buffer for the current plans: at the head of run(), before anything is
    // enqueued, whenever a plan override changed since the last sizing (one device sync, the old
    // buffer freed) -- no allocation or sync inside the step
    int size_wslabs();
    unsigned wslab_epoch = 0;  // plan_override_epoch() the slabs were last sized for
    // conv_wgrad_acc of layer i over its input and output gradient (after_gemm: recorded right
    // behind the GEMM launch), its combine deferred where defer_combine() holds and the slabs fit
    int wgrad_gemm(int i, const int8_t* x, const int8_t* dy, hipEvent_t after_gemm, hipStream_t st);

    // kernel probe: HIP events around one layer phase (0 fwd / 1 dgrad / 2 wgrad), up to ev0.size()
    // launches; where the events go is the driver's
    int probe_layer = -1, probe_phase = -1, probe_count = 0;
    std::vector<hipEvent_t> ev0, ev1;
    bool probe_paused = false;  // niti_model_probe_pause: the armed probe skips these launches
    bool probe_armed(int layer, int phase) const {
        return layer == probe_layer && phase == probe_phase && !probe_paused && !tuning && !capturing;
    }
    virtual void clear_probe();
    int set_probe(int layer, int phase, int max_launches);
    int probe_read(double* total_ms, int* count);
    // optional hipGraph replay of the single-device step: captured on an internal stream, fenced
    // against the caller's stream with events (the captured form and its key are the driver's)
    bool use_graph = false;
    hipStream_t gstream = nullptr;
    hipEvent_t gin = nullptr, gout = nullptr;
    int ensure_graph_stream();
    // evaluation (niti_model_eval_*): the driver's forward() and the head metrics of its logits, added
    // to the running totals; everything it needs is allocated in build() (alloc_eval)
    niti_eval_totals* ev_totals = nullptr;
    int32_t* ev_pred = nullptr;  // the last evaluation batch's predictions
    void* ev_ws = nullptr;
    size_t ev_ws_bytes = 0;
    int ev_topk = 5;
    bool eval_pass = false;  // forward() fills / copies by kernel (niti_map.hpp: fill_kernel)
    int alloc_eval();
    int eval_reset(hipStream_t st);
    int eval_read(niti_eval_totals* host_out, hipStream_t st);
    int get_predictions(int32_t* pred_host, hipStream_t st);
    int rowconv_error();
    // device-resident dataset steps (niti_model_*_steps_dataset): batch s of the dataset's order is
    // gathered (niti_dataset.hip) into the staging batch below -- allocated on first use, never inside
    // a step, and never moved, so a captured training step is captured once -- and goes through the
    // driver's own step() / eval() as any caller's uint8 batch; nothing on the host waits
    uint8_t* st_images = nullptr;
    int32_t* st_labels = nullptr;
    int steps_dataset(niti_dataset& ds, int64_t first_step, int n_steps, bool train, hipStream_t st);
    // training metrics (opt-in): head_metrics of each dataset training step's logits and staged
    // labels, added to totals of their own (allocated with the evaluation's, alloc_eval)
    bool tm_enabled = false;
    niti_eval_totals* tm_totals = nullptr;
    void* tm_ws = nullptr;
    int train_metrics_reset(hipStream_t st);
    int train_metrics_read(niti_eval_totals* host_out, hipStream_t st);
    // ---- update bits (include/niti_hip.h): one int32 per parameter layer, the bits of the gradient
    // its update keeps.  An allocation of its own (never among the range words, which every step
    // zeroes), 2 everywhere from build().  The update launches read it (SgdJob::rule = -(1 + layer)
    // with this table); only set_update_bits writes it, by kernel on the caller's stream, so a change
    // is ordered between enqueued steps and holds for replays of a captured step.  Autotuning, the
    // phase runs and the probe neither read nor write it.
    int32_t* upd_bits = nullptr;
    int alloc_update_bits();
    int set_update_bits(int layer, int bits, hipStream_t st);  // layer -1: every layer
    int get_update_bits(int32_t* bits_host, hipStream_t st);
    // the shared half of plan_set: the tile set {64, 128, 256} or the taps tile (own_tile: a tile of
    // the driver's own, which it vouches for), the strategy range, strategies 3 and 4 only for
    // unsplit activation GEMMs; then the override, with the split-K slabs it needs (gemm_slab)
    static int plan_op(int phase) { return phase == 0 ? PLAN_FWD : phase == 1 ? PLAN_DGRAD : PLAN_WGRAD; }
    static bool plan_valid(int op, const ConvGeom& g, const int plan[4], bool own_tile);
    int plan_commit(const PlanKey& k, int op, const int plan[4], bool gemm_slab);
    static int plan_out(const PlanChoice& c, int info[4]);

    // layer i's NITI_SGD job as both run()s build it: the update of w (a depthwise layer's in its
    // c_out = 1 form) with the int8 gradient where keep_grads, the derived copies it keeps in step
    // (wT where the caller says the GEMM input gradient reads it: wT_by_update; wf / wft, subw) and the
    // combine this step's weight gradient deferred (rule: the layer's update-bits word)
    SgdJob sgd_job(int i, bool wT_by_update) const;

    // ---- host access over P (each validates its layer itself)
    bool layer_ok(int layer) const { return layer >= 0 && layer < (int)P.size(); }
    int num_layers() const { return (int)P.size(); }
    int layer_info(int layer, int info[12]) const;
    // 1 a depthwise layer, 0 a dense one, -1 out of range
    int layer_depthwise(int layer) const { return layer_ok(layer) ? P[layer]->dw : -1; }
    // every derived copy p has, from w, on st: wT, subw, and the row kernels' wf / wft
    int refresh_copies(ParamLayer& p, hipStream_t st);
    // w from the host's OIHW (an im2col layer: through its columns), the scale, the derived copies
    virtual int set_weight(int layer, const int8_t* w_oihw_host, int wscale);
    int get_weight(int layer, int8_t* w_oihw_host);
    // copy_weights_from's loop, after the driver's own compatibility check: every layer's w and scale
    // device to device on st, then the derived copies
    int copy_layer_weights(const StepDriver& src, hipStream_t st);
    // off: the GEMM input gradients read IHWO16 copies the update skipped -- rebuilt here
    int set_rowconv(bool enable);
    // one tap to the host: src an NHWC16 activation / gradient of p's output (which 0 / 2) as NCHW, or
    // p.g8 (which 1) as OIHW; INVALID_VALUE for another `which`, for which 1 without g8_written and for
    // a short buffer, before anything is allocated or written
    int tap_out(const ParamLayer& p, int which, const int8_t* src, int8_t* host, size_t bytes);
    int get_logits(int8_t* host, int* exp_out, hipStream_t st);
    // every layer's forward and weight gradient, every input gradient but the first layer's (never run)
    int64_t step_macs() const;
    int spec_stats(uint32_t* out, int max_layers);
    // a layer's row-kernel state (grid barrier words + speculation slots; may be null)
    int spec_state(int layer, uint32_t** bar);

    // ---- what else the C ABI asks of a driver (each validates its layer / phase itself)
    // the layer's skip and gpool (only the chain driver has such layers)
    virtual int layer_skip(int layer, int* skip, int* gpool) const {
        if (!layer_ok(layer)) return NITI_INVALID_VALUE;
        *skip = *gpool = 0;
        return NITI_NO_ERROR;
    }
    // syncs st, refuses what the last step did not write, picks or rebuilds the source: then tap_out
    virtual int get_tap(int layer, int which, int8_t* host, size_t bytes, hipStream_t st) = 0;
    virtual int get_input(int8_t* host, int* ascale, hipStream_t st) = 0;
    // the logits as the last step left them on the device: int8 [batch][*ld], their exponent
    virtual void logits_view(const int8_t** logits, int* classes, int* ld, const int8_t** exp) const = 0;
    // x_nchw int8 with exponent exp_in, or (x_nchw == null) uint8 images through the on-device
    // input quantiser (MnistUtils.cpp:83-93)
    virtual int step(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st) = 0;
    virtual int eval(const int8_t* x_nchw, int exp_in, const uint8_t* images, const int32_t* labels, hipStream_t st) = 0;
    virtual int copy_weights_from(StepDriver& src, hipStream_t st) = 0;  // (another kind of driver: invalid)
    virtual int autotune(hipStream_t st, int reps) = 0;
    virtual int run_phase(int layer, int phase, hipStream_t st) = 0;
    virtual int plan_info(int layer, int phase, int info[4]) = 0;
    virtual int plan_set(int layer, int phase, const int plan[4]) = 0;
    virtual void set_overlap(bool enable) = 0;
    virtual void drop_graph() = 0;
    virtual int probe_alloc(int phase, int max_launches) { return NITI_NO_ERROR; }  // set_probe's extra
    virtual int probe_read_span(double* total_ms, int* count);  // (none unless the driver has a span probe)
    // Teardown.  The derived destructor goes first: its graphs, then (after synchronising cst) its own
    // events and side streams; here the probe events, cst synchronised, the shared events and the
    // graph stream, coll_grad, then coll, then cst itself; ws (device memory) last.
    virtual ~StepDriver();
};

// the concrete drivers (null and *rc set when build() fails)
std::unique_ptr<StepDriver> make_chain_driver(int arch, int batch, int in_hw, int* rc);
// a residual network of a stage list (ResNet-18's or the caller's), after resnet_check at its batch
std::unique_ptr<StepDriver> make_resnet_driver(const niti_resnet_spec* spec, int in_hw, int batch, int* rc);
// niti_model_resnet_check's rule (include/niti_hip.h) with the tensor-size bound taken at `batch`
int resnet_check(const niti_resnet_spec* spec, int in_hw, int batch, int* n_layers, int shapes[][8]);
// a chain model of the caller's layer list (NITI_ARCH_CHAIN), after chain_check at its batch.  rule: which
// entry points' rule holds -- CHAIN_RULE_PLAIN refuses stride != 1, CHAIN_RULE_STRIDED honours the layers'
// strides (niti_model_create_chain3), CHAIN_RULE_WIDE also takes gpool and up to NITI_CHAIN_MAX_LAYERS
// layers (niti_model_create_chain4); below CHAIN_RULE_WIDE the lists carry skip = gpool = 0
enum { CHAIN_RULE_PLAIN = 0, CHAIN_RULE_STRIDED = 1, CHAIN_RULE_WIDE = 2 };
std::unique_ptr<StepDriver> make_chain_list_driver(const niti_chain_layer3* layers, int n, int in_c, int in_hw, int batch,
                                                   int* rc, int rule);
// niti_model_chain_check's rule (include/niti_hip.h) with the tensor-size bound taken at `batch`
int chain_check(const niti_chain_layer3* layers, int n, int in_c, int in_hw, int batch, int shapes[][8], int rule);

// a first layer's weights as its im2col GEMM holds them: [co][kp], column (ky * KW + kx) * C_in + c,
// zero padded to the column pitch kp <-> OIHW
void cols_from_oihw(const ConvGeom& o, const int8_t* w, int8_t* wc, int kp);
void oihw_from_cols(const ConvGeom& o, const int8_t* wc, int8_t* w, int kp);

// ---------------------------------------------------------------------------- autotune harness
// min over three event-bracketed batches of `reps` back-to-back runs (no host sync inside)
struct TuneTimer {
    hipStream_t st = nullptr;
    int reps = 5;
    hipEvent_t ev[2] = {nullptr, nullptr};
    int init(hipStream_t st_, int reps_) {
        st = st_;
        reps = reps_;
        for (auto& e : ev)
            if (hipEventCreate(&e) != hipSuccess) return NITI_NO_EXECUTION;
        return NITI_NO_ERROR;
    }
    ~TuneTimer() {
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    template <class Run>
    int time(Run&& run, float* us) {
        int r = run();
        float best = 1e30f;
        for (int t = 0; t < 3 && r == NITI_NO_ERROR; ++t) {
            if (hipEventRecord(ev[0], st) != hipSuccess) return NITI_NO_EXECUTION;
            for (int k = 0; k < reps && r == NITI_NO_ERROR; ++k) r = run();
            if (hipEventRecord(ev[1], st) != hipSuccess || hipEventSynchronize(ev[1]) != hipSuccess)
                return NITI_NO_EXECUTION;
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[0], ev[1]) != hipSuccess) return NITI_NO_EXECUTION;
            best = std::min(best, ms * 1000.f / reps);
        }
        *us = best;
        return r;
    }
};

// Every GEMM-tile candidate of one plan key -- the tap-sharing weight-gradient kernel where it
// applies and 6 GEMM tile shapes, each x {store acc, recompute / the optional speculative pair /
// fused (activation GEMMs), split-K within steps / 2 and the workspace wsb} -- timed through
// `time(&us)` with the candidate set as the key's override, reported to `note(cand, us)`; a faster
// one replaces *best / *best_us.
template <class Time, class Note>
int tune_gemm_tiles(int op, const ConvGeom& g, size_t wsb, Time&& time, Note&& note, PlanChoice* best, float* best_us) {
    static const int tiles[7][2] = {{PLAN_TAPS_TILE, PLAN_TAPS_TILE}, {128, 128}, {128, 64}, {64, 128}, {64, 64},
                                    {256, 128}, {128, 256}};
    static const int split_opts[] = {2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64};
    const PlanKey key = conv_plan_key(op, g);
    const int k_step = conv_plan_k_step(op, g);
    const int steps = (key.K + k_step - 1) / k_step;
    const bool act = op != PLAN_WGRAD;
    const bool taps = op == PLAN_WGRAD && conv_wgrad_taps_ok(g);
    for (const auto& t : tiles) {
        if (t[0] == PLAN_TAPS_TILE && !taps) continue;
        std::vector<PlanChoice> cands;
        PlanChoice c;
        c.bm = t[0];
        c.bn = t[1];
        c.splits = 1;
        c.strat = 0;
        cands.push_back(c);
        if (act) {
            c.strat = 1;
            cands.push_back(c);
            // the speculative pair only on request (NITI_TUNE_SPEC=1): timed here on one
            // batch its guess always holds, but over a run of batches 60-80 % of the deep
            // layers' pairs miss (profiles/r05_gemm_spec.txt) and then cost more than STORE
            if (tune_spec()) {
                c.strat = 3;
                cands.push_back(c);
            }
            c.strat = 4;  // one launch, the rescale fused (where every tile is resident)
            cands.push_back(c);
        }
        for (int s : split_opts) {
            if (s > steps / 2 || plan_slab_bytes(key.M, key.N, s) > wsb) break;
            c.strat = 2;
            c.splits = s;
            cands.push_back(c);
        }
        for (const PlanChoice& cand : cands) {
            plan_override_set(key, cand);
            float us = 0.f;
            const int rc = time(&us);
            note(cand, us);
            if (rc != NITI_NO_ERROR) return rc;
            if (us < *best_us) {
                *best_us = us;
                *best = cand;
            }
        }
    }
    return NITI_NO_ERROR;
}

}  // namespace niti
