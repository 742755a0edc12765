// niti_model_capi.hip -- the niti_model_* C ABI (section 3 of include/niti_hip.h) over a StepDriver
// (niti_step_driver.hpp): the chain driver (LeNet / VGG-11 / VGG-16 or the caller's layer list,
// niti_model.hip) or ResNet-18 (niti_resnet_model.hip), chosen once in niti_model_create3 /
// niti_model_create_chain.  Every entry point checks its handle
// and pointers, then makes one call; layers and phases are the driver's to check.
#include <rccl/rccl.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/niti_hip.h"
#include "niti_step_driver.hpp"

struct niti_model {
    std::unique_ptr<niti::StepDriver> d;
};

extern "C" {

int niti_model_create(int arch, int batch, niti_model_t* out) { return niti_model_create2(arch, batch, 0, out); }

int niti_model_create2(int arch, int batch, int in_hw, niti_model_t* out) {
    return niti_model_create3(arch, batch, in_hw, 0, out);
}

int niti_model_create3(int arch, int batch, int in_hw, int classes, niti_model_t* out) {
    if (!out || batch <= 0 || in_hw < 0 || classes < 0) return NITI_INVALID_VALUE;
    int rc = NITI_NO_ERROR;
    std::unique_ptr<niti::StepDriver> d;
    if (arch == NITI_ARCH_RESNET18) {  // the stage list of ResNet-18, built as any other
        if (classes > 2048) return NITI_INVALID_VALUE;
        const niti_resnet_spec spec = {3, 7, 2, 3, 1, 64, 4, {2, 2, 2, 2}, classes > 0 ? classes : 1000};
        d = niti::make_resnet_driver(&spec, in_hw > 0 ? in_hw : 224, batch, &rc);
    } else if (classes != 0)  // the LeNet / VGG heads are fixed (10 or 1000 classes)
        return NITI_NOT_SUPPORT;
    else
        d = niti::make_chain_driver(arch, batch, in_hw, &rc);
    if (rc != NITI_NO_ERROR) return rc;
    *out = new niti_model{std::move(d)};
    return NITI_NO_ERROR;
}

int niti_model_chain_check4(const niti_chain_layer3* layers, int n, int in_c, int in_hw, int shapes[][8]) {
    return niti::chain_check(layers, n, in_c, in_hw, 1, shapes, niti::CHAIN_RULE_WIDE);
}

static int create_chain(const niti_chain_layer3* layers, int n, int in_c, int in_hw, int batch, int rule, niti_model_t* out) {
    if (!out || batch <= 0) return NITI_INVALID_VALUE;
    int rc = NITI_NO_ERROR;
    std::unique_ptr<niti::StepDriver> d = niti::make_chain_list_driver(layers, n, in_c, in_hw, batch, &rc, rule);
    if (!d) return rc;
    *out = new niti_model{std::move(d)};
    return NITI_NO_ERROR;
}

int niti_model_create_chain4(const niti_chain_layer3* layers, int n, int in_c, int in_hw, int batch, niti_model_t* out) {
    return create_chain(layers, n, in_c, in_hw, batch, niti::CHAIN_RULE_WIDE, out);
}

// the eight-field list as the same list with skip = gpool = 0 (empty where the arguments are malformed:
// the check then refuses them as it always did)
static std::vector<niti_chain_layer3> chain_layers3(const niti_chain_layer2* layers, int n) {
    std::vector<niti_chain_layer3> t;
    for (int i = 0; layers != nullptr && i < n; ++i) {
        const niti_chain_layer2& l = layers[i];
        t.push_back({l.c_out, l.kernel, l.stride, l.pad, l.relu, l.pool, l.flatten, l.depthwise, 0, 0});
    }
    return t;
}

int niti_model_chain_check2(const niti_chain_layer2* layers, int n, int in_c, int in_hw, int shapes[][8]) {
    const std::vector<niti_chain_layer3> t = chain_layers3(layers, n);
    return niti::chain_check(t.empty() ? nullptr : t.data(), n, in_c, in_hw, 1, shapes, niti::CHAIN_RULE_PLAIN);
}

int niti_model_create_chain2(const niti_chain_layer2* layers, int n, int in_c, int in_hw, int batch, niti_model_t* out) {
    const std::vector<niti_chain_layer3> t = chain_layers3(layers, n);
    return create_chain(t.empty() ? nullptr : t.data(), n, in_c, in_hw, batch, niti::CHAIN_RULE_PLAIN, out);
}

int niti_model_chain_check3(const niti_chain_layer2* layers, int n, int in_c, int in_hw, int shapes[][8]) {
    const std::vector<niti_chain_layer3> t = chain_layers3(layers, n);
    return niti::chain_check(t.empty() ? nullptr : t.data(), n, in_c, in_hw, 1, shapes, niti::CHAIN_RULE_STRIDED);
}

int niti_model_create_chain3(const niti_chain_layer2* layers, int n, int in_c, int in_hw, int batch, niti_model_t* out) {
    const std::vector<niti_chain_layer3> t = chain_layers3(layers, n);
    return create_chain(t.empty() ? nullptr : t.data(), n, in_c, in_hw, batch, niti::CHAIN_RULE_STRIDED, out);
}

// the seven-field list as the same list with depthwise = 0 (empty where the arguments are malformed:
// the check then refuses them as it always did)
static std::vector<niti_chain_layer2> chain_layers2(const niti_chain_layer* layers, int n) {
    std::vector<niti_chain_layer2> t;
    for (int i = 0; layers != nullptr && i < n; ++i) {
        const niti_chain_layer& l = layers[i];
        t.push_back({l.c_out, l.kernel, l.stride, l.pad, l.relu, l.pool, l.flatten, 0});
    }
    return t;
}

int niti_model_chain_check(const niti_chain_layer* layers, int n, int in_c, int in_hw, int shapes[][8]) {
    const std::vector<niti_chain_layer2> t = chain_layers2(layers, n);
    return niti_model_chain_check2(t.empty() ? nullptr : t.data(), n, in_c, in_hw, shapes);
}

int niti_model_create_chain(const niti_chain_layer* layers, int n, int in_c, int in_hw, int batch, niti_model_t* out) {
    const std::vector<niti_chain_layer2> t = chain_layers2(layers, n);
    return niti_model_create_chain2(t.empty() ? nullptr : t.data(), n, in_c, in_hw, batch, out);
}

int niti_model_resnet_check(const niti_resnet_spec* spec, int in_hw, int* n_layers, int shapes[][8]) {
    return niti::resnet_check(spec, in_hw, 1, n_layers, shapes);
}

int niti_model_create_resnet(const niti_resnet_spec* spec, int in_hw, int batch, niti_model_t* out) {
    if (!out || batch <= 0) return NITI_INVALID_VALUE;
    int rc = NITI_NO_ERROR;
    std::unique_ptr<niti::StepDriver> d = niti::make_resnet_driver(spec, in_hw, batch, &rc);
    if (rc != NITI_NO_ERROR) return rc;
    *out = new niti_model{std::move(d)};
    return NITI_NO_ERROR;
}

void niti_model_destroy(niti_model_t m) { delete m; }

int niti_model_num_layers(niti_model_t m) { return m ? m->d->num_layers() : 0; }

int niti_model_layer_info(niti_model_t m, int layer, int info[12]) {
    return m && info ? m->d->layer_info(layer, info) : NITI_INVALID_VALUE;
}

int niti_model_layer_depthwise(niti_model_t m, int layer) { return m ? m->d->layer_depthwise(layer) : -1; }

int niti_model_layer_skip(niti_model_t m, int layer, int* skip, int* gpool) {
    return m && skip && gpool ? m->d->layer_skip(layer, skip, gpool) : NITI_INVALID_VALUE;
}

int niti_model_set_weight(niti_model_t m, int layer, const int8_t* w_host, int wscale) {
    return m ? m->d->set_weight(layer, w_host, wscale) : NITI_INVALID_VALUE;
}

int niti_model_get_weight(niti_model_t m, int layer, int8_t* w_host) {
    return m ? m->d->get_weight(layer, w_host) : NITI_INVALID_VALUE;
}

int niti_model_train_step(niti_model_t m, const int8_t* x_nchw, int exp_in, const int32_t* labels, void* stream) {
    if (!m || !x_nchw || !labels) return NITI_INVALID_VALUE;
    return m->d->step(x_nchw, exp_in, nullptr, labels, (hipStream_t)stream);
}

int niti_model_train_step_images(niti_model_t m, const uint8_t* images_nchw, const int32_t* labels, void* stream) {
    if (!m || !images_nchw || !labels) return NITI_INVALID_VALUE;
    return m->d->step(nullptr, 0, images_nchw, labels, (hipStream_t)stream);
}

int niti_model_eval_step(niti_model_t m, const int8_t* x_nchw, int exp_in, const int32_t* labels, void* stream) {
    if (!m || !x_nchw || !labels) return NITI_INVALID_VALUE;
    return m->d->eval(x_nchw, exp_in, nullptr, labels, (hipStream_t)stream);
}

int niti_model_eval_step_images(niti_model_t m, const uint8_t* images_nchw, const int32_t* labels, void* stream) {
    if (!m || !images_nchw || !labels) return NITI_INVALID_VALUE;
    return m->d->eval(nullptr, 0, images_nchw, labels, (hipStream_t)stream);
}

int niti_model_eval_reset(niti_model_t m, void* stream) {
    return m ? m->d->eval_reset((hipStream_t)stream) : NITI_INVALID_VALUE;
}

int niti_model_eval_read(niti_model_t m, niti_eval_totals* host_out, void* stream) {
    return m && host_out ? m->d->eval_read(host_out, (hipStream_t)stream) : NITI_INVALID_VALUE;
}

int niti_model_eval_topk(niti_model_t m, int k) {
    if (!m || k < 1) return NITI_INVALID_VALUE;
    m->d->ev_topk = k;  // (clamped to the class count at each step)
    return NITI_NO_ERROR;
}

int niti_model_get_predictions(niti_model_t m, int32_t* pred_host, void* stream) {
    return m && pred_host ? m->d->get_predictions(pred_host, (hipStream_t)stream) : NITI_INVALID_VALUE;
}

int niti_model_train_steps_dataset(niti_model_t m, niti_dataset_t ds, int64_t first_step, int n_steps, void* stream) {
    if (!m || !ds) return NITI_INVALID_VALUE;
    return m->d->steps_dataset(*ds, first_step, n_steps, true, (hipStream_t)stream);
}

int niti_model_eval_steps_dataset(niti_model_t m, niti_dataset_t ds, int64_t first_step, int n_steps, void* stream) {
    if (!m || !ds) return NITI_INVALID_VALUE;
    return m->d->steps_dataset(*ds, first_step, n_steps, false, (hipStream_t)stream);
}

int niti_model_train_metrics(niti_model_t m, int enable) {
    if (!m) return NITI_INVALID_VALUE;
    m->d->tm_enabled = enable != 0;
    return NITI_NO_ERROR;
}

int niti_model_train_metrics_reset(niti_model_t m, void* stream) {
    return m ? m->d->train_metrics_reset((hipStream_t)stream) : NITI_INVALID_VALUE;
}

int niti_model_train_metrics_read(niti_model_t m, niti_eval_totals* host_out, void* stream) {
    return m && host_out ? m->d->train_metrics_read(host_out, (hipStream_t)stream) : NITI_INVALID_VALUE;
}

int niti_model_copy_weights(niti_model_t dst, niti_model_t src, void* stream) {
    return dst && src ? dst->d->copy_weights_from(*src->d, (hipStream_t)stream) : NITI_INVALID_VALUE;
}

int niti_model_set_update_bits(niti_model_t m, int layer, int bits, void* stream) {
    return m ? m->d->set_update_bits(layer, bits, (hipStream_t)stream) : NITI_INVALID_VALUE;
}

int niti_model_get_update_bits(niti_model_t m, int32_t* bits_host, void* stream) {
    return m && bits_host ? m->d->get_update_bits(bits_host, (hipStream_t)stream) : NITI_INVALID_VALUE;
}

int niti_model_get_input(niti_model_t m, int8_t* x_nchw_host, int* ascale, void* stream) {
    return m && x_nchw_host ? m->d->get_input(x_nchw_host, ascale, (hipStream_t)stream) : NITI_INVALID_VALUE;
}

int niti_model_get_logits(niti_model_t m, int8_t* logits_host, int* exp_out, void* stream) {
    return m && logits_host ? m->d->get_logits(logits_host, exp_out, (hipStream_t)stream) : NITI_INVALID_VALUE;
}

int niti_model_get_tap(niti_model_t m, int layer, int which, int8_t* host, size_t bytes, void* stream) {
    return m && host ? m->d->get_tap(layer, which, host, bytes, (hipStream_t)stream) : NITI_INVALID_VALUE;
}

int64_t niti_model_step_macs(niti_model_t m) { return m ? m->d->step_macs() : 0; }

int niti_model_set_overlap(niti_model_t m, int enable) {
    if (!m) return NITI_INVALID_VALUE;
    m->d->set_overlap(enable != 0);
    return NITI_NO_ERROR;
}

int niti_model_keep_grads(niti_model_t m, int enable) {
    if (!m) return NITI_INVALID_VALUE;
    m->d->keep_grads = enable != 0;
    m->d->drop_graph();
    return NITI_NO_ERROR;
}

int niti_model_set_rowconv(niti_model_t m, int enable) { return m ? m->d->set_rowconv(enable != 0) : NITI_INVALID_VALUE; }

int niti_model_spec_slot(niti_model_t m, int layer, int dgrad, uint32_t* out32) {
    uint32_t* bar = nullptr;
    if (!m || !out32 || m->d->spec_state(layer, &bar) != NITI_NO_ERROR) return NITI_INVALID_VALUE;
    std::fill(out32, out32 + 32, 0u);
    if (bar == nullptr) return NITI_NO_ERROR;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(out32, niti::rowconv_spec_slot(bar, dgrad != 0), 32 * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return NITI_NO_EXECUTION;
    return NITI_NO_ERROR;
}

int niti_model_spec_stats(niti_model_t m, uint32_t* out, int max_layers) {
    return m && out && max_layers >= 0 ? m->d->spec_stats(out, max_layers) : NITI_INVALID_VALUE;
}

int niti_model_rowconv_error(niti_model_t m) { return m ? m->d->rowconv_error() : NITI_INVALID_VALUE; }

int niti_model_set_graph(niti_model_t m, int enable) {
    if (!m) return NITI_INVALID_VALUE;
    m->d->drop_graph();
    m->d->use_graph = enable != 0;
    return NITI_NO_ERROR;
}

int niti_model_autotune(niti_model_t m, int reps, void* stream) {
    return m ? m->d->autotune((hipStream_t)stream, reps) : NITI_INVALID_VALUE;
}

int niti_model_run_phase(niti_model_t m, int layer, int phase, void* stream) {
    return m ? m->d->run_phase(layer, phase, (hipStream_t)stream) : NITI_INVALID_VALUE;
}

int niti_model_plan_info(niti_model_t m, int layer, int phase, int info[4]) {
    return m && info ? m->d->plan_info(layer, phase, info) : NITI_INVALID_VALUE;
}

int niti_model_plan_set(niti_model_t m, int layer, int phase, const int plan[4]) {
    return m ? m->d->plan_set(layer, phase, plan) : NITI_INVALID_VALUE;
}

void niti_plan_reset(void) { niti::plan_override_clear_all(); }

int niti_model_set_probe(niti_model_t m, int layer, int phase, int max_launches) {
    return m && max_launches >= 0 ? m->d->set_probe(layer, phase, max_launches) : NITI_INVALID_VALUE;
}

int niti_model_probe_read_span(niti_model_t m, double* total_ms, int* count) {
    return m && total_ms && count ? m->d->probe_read_span(total_ms, count) : NITI_INVALID_VALUE;
}

int niti_model_probe_pause(niti_model_t m, int paused) {
    if (!m) return NITI_INVALID_VALUE;
    m->d->probe_paused = paused != 0;
    return NITI_NO_ERROR;
}

int niti_model_probe_read(niti_model_t m, double* total_ms, int* count) {
    return m && total_ms && count ? m->d->probe_read(total_ms, count) : NITI_INVALID_VALUE;
}

int niti_dp_get_unique_id(char id[NITI_UNIQUE_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == NITI_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return NITI_NO_EXECUTION;
    memcpy(id, &u, sizeof(u));
    return NITI_NO_ERROR;
}

int niti_model_attach_comm(niti_model_t m, const char id[NITI_UNIQUE_ID_BYTES], int rank, int world, int exact) {
    if (!m || !id || world < 1 || rank < 0 || rank >= world) return NITI_INVALID_VALUE;
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    // the split-agreement flag and stream first: a local allocation failure then returns before any
    // collective call, instead of leaving the peers blocked in one this rank never enters
    int32_t* flag = nullptr;
    hipStream_t ast = nullptr;
    if (hipMalloc(&flag, sizeof(int32_t)) != hipSuccess || hipStreamCreate(&ast) != hipSuccess) {
        if (flag) (void)hipFree(flag);
        return NITI_OUT_OF_MEMORY;
    }
    auto c = std::make_unique<niti::RcclCollective>();
    if (ncclCommInitRank(&c->comm, world, u, rank) != ncclSuccess) {
        (void)hipFree(flag);
        (void)hipStreamDestroy(ast);
        return NITI_NO_EXECUTION;
    }
    c->world = world;
    // the gradient communicator: split off the first (collective over the ranks), its own
    // resources, so its SUMs and the ranges' MAXes are not serialised against each other
    auto cg = std::make_unique<niti::RcclCollective>();
    const bool split_ok = ncclCommSplit(c->comm, 0, rank, &cg->comm, nullptr) == ncclSuccess;
    // every rank must pick the same mode (the SUMs run on different communicators and streams in
    // the two modes): agree on the split's success with a MIN over the range communicator, which
    // every rank enters whatever its own split did
    int32_t ok = split_ok ? 1 : 0;
    const bool agreed = hipMemcpyAsync(flag, &ok, sizeof(ok), hipMemcpyHostToDevice, ast) == hipSuccess &&
                        ncclAllReduce(flag, flag, 1, ncclInt32, ncclMin, c->comm, ast) == ncclSuccess &&
                        hipMemcpyAsync(&ok, flag, sizeof(ok), hipMemcpyDeviceToHost, ast) == hipSuccess &&
                        hipStreamSynchronize(ast) == hipSuccess;
    (void)hipFree(flag);
    (void)hipStreamDestroy(ast);
    if (!agreed) {
        if (split_ok) (void)ncclCommDestroy(cg->comm);
        cg->comm = nullptr;
        (void)ncclCommDestroy(c->comm);
        c->comm = nullptr;
        return NITI_NO_EXECUTION;
    }
    bool shared = false;
    if (ok == 0) {
        // some rank has no split: every rank's gradient SUMs use the range communicator, in the
        // step's program order
        if (split_ok) (void)ncclCommDestroy(cg->comm);
        cg->comm = c->comm;
        cg->owns = false;
        shared = true;
    }
    cg->world = world;
    m->d->attach(std::move(c), std::move(cg), shared, world, rank, exact);
    return NITI_NO_ERROR;
}

struct niti_local_group {
    std::shared_ptr<niti::LocalGroup> g;
};

int niti_local_group_create(int world, niti_local_group_t* out) {
    if (!out || world < 1 || world > niti::LocalGroup::MAX_RANKS) return NITI_INVALID_VALUE;
    auto* h = new niti_local_group();
    h->g = std::make_shared<niti::LocalGroup>();
    h->g->world = world;
    if (hipStreamCreateWithFlags(&h->g->rst, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return NITI_NO_EXECUTION;
    }
    *out = h;
    return NITI_NO_ERROR;
}

void niti_local_group_destroy(niti_local_group_t g) { delete g; }

int niti_model_attach_local(niti_model_t m, niti_local_group_t g, int rank, int exact) {
    if (!m || !g || rank < 0 || rank >= g->g->world) return NITI_INVALID_VALUE;
    auto c = std::make_unique<niti::LocalCollective>();
    c->g = g->g;
    c->rank = rank;
    c->chan = 0;
    auto cg = std::make_unique<niti::LocalCollective>();
    cg->g = g->g;
    cg->rank = rank;
    // NITI_DIAG_SHARED_COMM=1 (tests): the gradient SUMs on the range channel, as attach_comm's
    // no-split fallback runs them on one RCCL communicator
    const bool shared = getenv("NITI_DIAG_SHARED_COMM") != nullptr;
    cg->chan = shared ? 0 : 1;
    m->d->attach(std::move(c), std::move(cg), shared, g->g->world, rank, exact);
    return NITI_NO_ERROR;
}

}  // extern "C"
