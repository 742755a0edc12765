// niti_capi.hip -- extern "C" entry points of sections 1 and 2 of include/niti_hip.h.
#include "../../include/niti_hip.h"
#include <memory>
#include <vector>

#include "niti_internal.hpp"
#include "niti_kernels.hpp"

// Host tensors: MNN's CPU backend hands Executions Tensor::host<T>() pointers
// (source/core/Execution.hpp:24-82, express/Executor.cpp:559-569).  Any tensor whose pointer is
// not device memory (hipPointerGetAttributes) is staged through a device buffer the handle keeps:
// inputs and outputs copied in before onExecute, outputs copied back after, and the call returns
// once the host outputs are written (the CPU backend's onExecute is synchronous).
struct niti_execution {
    niti::Execution* impl = nullptr;
    int op = 0;
    std::vector<void*> stage;
    std::vector<size_t> stage_bytes;
    uint32_t* err_host = nullptr;  // pinned copy of the Execution's error word (synchronous calls)
    ~niti_execution() {
        delete impl;
        for (void* p : stage)
            if (p) (void)hipFree(p);
        if (err_host) (void)hipHostFree(err_host);
    }
};

namespace {
int code(hipError_t e) {
    if (e == hipSuccess) return NITI_NO_ERROR;
    if (e == hipErrorOutOfMemory) return NITI_OUT_OF_MEMORY;
    if (e == hipErrorInvalidValue) return NITI_INVALID_VALUE;
    return NITI_NO_EXECUTION;
}
// false when ConvGeom::finalize rejects the geometry (callers return COMPUTE_SIZE_ERROR)
bool to_geom(const niti_geom* g, niti::ConvGeom* out) {
    niti::ConvGeom& r = *out;
    r = niti::ConvGeom{};
    r.n = g->n;
    r.c_in = g->c_in;
    r.h = g->h;
    r.w = g->w;
    r.c_out = g->c_out;
    r.kh = g->kh;
    r.kw = g->kw;
    r.sh = g->stride_h;
    r.sw = g->stride_w;
    r.pt = g->pad_t;
    r.pl = g->pad_l;
    r.pb = g->pad_b;
    r.pr = g->pad_r;
    r.dh = g->dilate_h;
    r.dw = g->dilate_w;
    return r.finalize();
}
inline hipStream_t S(void* s) { return (hipStream_t)s; }
// true for pageable or pinned host memory (anything hipPointerGetAttributes does not report as
// device or managed memory)
bool is_host_pointer(const void* p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    return a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged;
}

// bytes of one Execution tensor: int8 elements, NC4HW4 with the channel count rounded up to 4
// (MNN's CPU layout [ceil(C/4)][N][H][W][4]); the loss gradient's one-hot target and the
// transpose's permutation are int32
size_t tensor_bytes(int op, bool is_out, int idx, const niti_tensor& t) {
    int64_t d[4];
    for (int k = 0; k < 4; ++k) {
        if (t.dims[k] < 0) return 0;
        d[k] = t.dims[k];
    }
    if (!is_out && idx == 2 &&
        (op == NITI_OP_LOSS_GRAD_INT8 || op == NITI_OP_DSP_LOSSGRAD_INT8 || op == NITI_OP_LOSS_INT8))
        return (size_t)(d[0] * d[1] * d[2] * d[3] * 4);
    if (is_out && idx == 0 && op == NITI_OP_LOSS_INT8) return sizeof(float);  // the loss scalar
    if (!is_out && idx == 1 && op == NITI_OP_DSP_TRANSPOSE_INT8) return 4 * sizeof(int32_t);
    if (t.format == NITI_FORMAT_NC4HW4) return (size_t)(d[0] * ((d[1] + 3) / 4) * 4 * d[2] * d[3]);
    return (size_t)(d[0] * d[1] * d[2] * d[3]);
}

// The Execution's error word after `st` completes: NITI_NO_EXECUTION (and the word cleared) if a
// launch flagged invalid results, else NITI_NO_ERROR.  copied: the word was already copied into
// err_host on `st` (the staged path enqueues that copy before its synchronize).
int take_error(niti_execution* e, hipStream_t st, bool copied) {
    uint32_t* dev = e->impl->errorFlag();
    if (dev == nullptr) return NITI_NO_ERROR;
    uint32_t v = 0;
    if (copied) {
        v = *e->err_host;
    } else if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(&v, dev, 4, hipMemcpyDeviceToHost) != hipSuccess) {
        return NITI_NO_EXECUTION;
    }
    if (v == 0) return NITI_NO_ERROR;
    (void)hipMemsetAsync(dev, 0, 4, st);
    (void)hipStreamSynchronize(st);
    return NITI_NO_EXECUTION;
}
}  // namespace

extern "C" {

const char* niti_version(void) { return "niti-mi355x 0.1 (gfx950, int8 MFMA v_mfma_i32_32x32x32_i8)"; }

// ------------------------------------------------------------------ section 1
int niti_create_execution(int op_type, const niti_conv2d_common* common, niti_execution_t* out) {
    if (!out) return NITI_INVALID_VALUE;
    int err = NITI_NO_ERROR;
    niti::Execution* e = niti::create_execution(op_type, common, &err);
    if (!e) return err;
    auto* h = new niti_execution();
    h->impl = e;
    h->op = op_type;
    *out = h;
    return NITI_NO_ERROR;
}

int niti_execution_resize(niti_execution_t e, const niti_tensor* in, int nin, const niti_tensor* out, int nout) {
    if (!e || !in || !out) return NITI_INVALID_VALUE;
    return e->impl->onResize(in, nin, out, nout);
}

int niti_execution_execute(niti_execution_t e, const niti_tensor* in, int nin, const niti_tensor* out, int nout,
                           void* stream) {
    if (!e || !in || !out || nin < 0 || nout < 0) return NITI_INVALID_VALUE;
    const hipStream_t st = S(stream);
    bool any_host = false;
    for (int i = 0; i < nin + nout && !any_host; ++i) {
        const niti_tensor& t = i < nin ? in[i] : out[i - nin];
        any_host = t.data != nullptr && is_host_pointer(t.data);
    }
    if (!any_host) return e->impl->onExecute(in, nin, out, nout, st);
    // stage every host tensor through the handle's device buffers
    std::vector<niti_tensor> di(in, in + nin), dout(out, out + nout);
    if (e->stage.size() < (size_t)(nin + nout)) {
        e->stage.resize(nin + nout, nullptr);
        e->stage_bytes.resize(nin + nout, 0);
    }
    for (int i = 0; i < nin + nout; ++i) {
        const bool is_out = i >= nin;
        niti_tensor& t = is_out ? dout[i - nin] : di[i];
        if (t.data == nullptr || !is_host_pointer(t.data)) continue;
        const size_t bytes = tensor_bytes(e->op, is_out, is_out ? i - nin : i, t);
        if (bytes == 0) return NITI_INVALID_VALUE;
        if (e->stage_bytes[i] < bytes) {
            if (e->stage[i]) (void)hipFree(e->stage[i]);
            e->stage[i] = nullptr;
            e->stage_bytes[i] = 0;
            if (hipMalloc(&e->stage[i], bytes) != hipSuccess) return NITI_OUT_OF_MEMORY;
            e->stage_bytes[i] = bytes;
        }
        // outputs too: an Execution may leave parts of its output untouched (pad lanes, scalars)
        if (hipMemcpyAsync(e->stage[i], t.data, bytes, hipMemcpyHostToDevice, st) != hipSuccess)
            return NITI_NO_EXECUTION;
        t.data = e->stage[i];
    }
    const int rc = e->impl->onExecute(di.data(), nin, dout.data(), nout, st);
    if (rc != NITI_NO_ERROR) return rc;
    for (int k = 0; k < nout; ++k)
        if (dout[k].data != out[k].data &&
            hipMemcpyAsync(out[k].data, dout[k].data, tensor_bytes(e->op, true, k, out[k]), hipMemcpyDeviceToHost,
                           st) != hipSuccess)
            return NITI_NO_EXECUTION;
    // a synchronous call returns its ErrorCode (ErrorCode.hpp:17-30): a launch that flagged its
    // results invalid (the fused barrier's timeout) is NO_EXECUTION, not NO_ERROR
    uint32_t* flag = e->impl->errorFlag();
    if (flag != nullptr) {
        if (e->err_host == nullptr && hipHostMalloc((void**)&e->err_host, sizeof(uint32_t)) != hipSuccess) {
            e->err_host = nullptr;
            return NITI_OUT_OF_MEMORY;
        }
        if (hipMemcpyAsync(e->err_host, flag, 4, hipMemcpyDeviceToHost, st) != hipSuccess) return NITI_NO_EXECUTION;
    }
    if (hipStreamSynchronize(st) != hipSuccess) return NITI_NO_EXECUTION;
    return take_error(e, st, flag != nullptr);
}

int niti_execution_status(niti_execution_t e, void* stream) {
    if (!e) return NITI_INVALID_VALUE;
    return take_error(e, S(stream), false);
}

void niti_destroy_execution(niti_execution_t e) { delete e; }

size_t niti_execution_workspace_bytes(niti_execution_t e) { return e ? e->impl->workspaceBytes() : 0; }

int niti_tensor_convert(const niti_tensor* src, const niti_tensor* dst, void* stream) {
    if (!src || !dst) return NITI_INVALID_VALUE;
    return niti::convert_tensor(*src, *dst, S(stream));
}

// ------------------------------------------------------------------ section 2
int niti_geom_finalize(niti_geom* g) {
    if (!g) return NITI_INVALID_VALUE;
    niti::ConvGeom r{};
    r.n = g->n;
    r.c_in = g->c_in;
    r.h = g->h;
    r.w = g->w;
    r.c_out = g->c_out;
    r.kh = g->kh;
    r.kw = g->kw;
    r.sh = g->stride_h;
    r.sw = g->stride_w;
    r.pt = g->pad_t;
    r.pl = g->pad_l;
    r.pb = g->pad_b;
    r.pr = g->pad_r;
    r.dh = g->dilate_h;
    r.dw = g->dilate_w;
    if (!r.finalize()) return NITI_COMPUTE_SIZE_ERROR;
    g->oh = r.oh;
    g->ow = r.ow;
    g->cip = r.cip;
    g->cop = r.cop;
    g->np = r.np;
    return NITI_NO_ERROR;
}

int niti_conv_workspace_bytes(const niti_geom* g, int op, size_t* bytes) {
    if (!g || !bytes) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    if (op == 0)
        *bytes = niti::conv_fwd_workspace(r);
    else if (op == 1)
        *bytes = niti::conv_dgrad_workspace(r);
    else if (op == 2)
        *bytes = niti::conv_wgrad_workspace(r);
    else
        return NITI_INVALID_VALUE;
    return NITI_NO_ERROR;
}

int niti_conv_plan_set(const niti_geom* g, int op, const int plan[4]) {
    if (!g || op < 0 || op > 2) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    const int pop = op == 0 ? niti::PLAN_FWD : op == 1 ? niti::PLAN_DGRAD : niti::PLAN_WGRAD;
    const niti::PlanKey k = niti::conv_plan_key(pop, r);
    if (plan == nullptr) {
        niti::plan_override_clear(k);
        return NITI_NO_ERROR;
    }
    auto tile_ok = [](int t) { return t == 64 || t == 128 || t == 256; };
    const bool taps = plan[0] == niti::PLAN_TAPS_TILE && plan[1] == niti::PLAN_TAPS_TILE && pop == niti::PLAN_WGRAD &&
                      niti::conv_wgrad_taps_ok(r);
    if ((!taps && (!tile_ok(plan[0]) || !tile_ok(plan[1]))) || plan[2] < 1 || plan[2] > 4096 || plan[3] < 0 ||
        plan[3] > 4 || (taps && plan[3] == 1) || (plan[3] >= 3 && (pop == niti::PLAN_WGRAD || plan[2] != 1)))
        return NITI_INVALID_VALUE;
    niti::PlanChoice c;
    c.bm = plan[0];
    c.bn = plan[1];
    c.splits = plan[2];
    c.strat = plan[3];
    niti::plan_override_set(k, c);
    return NITI_NO_ERROR;
}

int niti_conv_plan_info(const niti_geom* g, int op, size_t ws_bytes, int info[4]) {
    if (!g || !info || op < 0 || op > 2) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_INVALID_VALUE;
    const int pop = op == 0 ? niti::PLAN_FWD : op == 1 ? niti::PLAN_DGRAD : niti::PLAN_WGRAD;
    const niti::PlanChoice c = niti::conv_plan_query(pop, r, op != 2, ws_bytes);
    info[0] = c.bm;
    info[1] = c.bn;
    info[2] = c.splits;
    info[3] = c.strat;
    return NITI_NO_ERROR;
}

int niti_matmul_workspace_bytes(int m, int ldc, int k16, size_t* bytes) {
    if (!bytes || ldc % 16 || k16 % 16) return NITI_INVALID_VALUE;
    *bytes = niti::matmul_workspace(m, ldc, k16);
    return NITI_NO_ERROR;
}

int niti_conv_fwd_acc(const niti_geom* g, const int8_t* x, const int8_t* w, int32_t* acc, uint32_t* amax, void* ws,
                      size_t ws_bytes, void* stream) {
    if (!g) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    return code(niti::conv_fwd_acc(r, x, w, acc, amax, ws, ws_bytes, S(stream)));
}

int niti_conv_dgrad_acc(const niti_geom* g, const int8_t* dy, const int8_t* wt, int32_t* acc, uint32_t* amax,
                        void* ws, size_t ws_bytes, void* stream) {
    if (!g) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    return code(niti::conv_dgrad_acc(r, dy, wt, acc, amax, ws, ws_bytes, S(stream)));
}

static niti::ActOut act_out(const int8_t* exp_in, const int8_t* wscale, int8_t* exp_out, int relu,
                            const int8_t* relu_mask, int8_t* out) {
    niti::ActOut o;
    o.out = out;
    o.relu = relu;
    o.relu_mask = relu_mask;
    o.exp_in = exp_in;
    o.wscale = wscale;
    o.exp_out = exp_out;
    return o;
}

int niti_conv_rows_ok(const niti_geom* g) {
    niti::ConvGeom r;
    return g && to_geom(g, &r) && niti::rowconv_ok(r) ? 1 : 0;
}

int niti_conv_rows_plan(const niti_geom* g, int dgrad, int* W, int* R, int* ks, int* workgroups) {
    niti::ConvGeom r, d;
    if (!g || !W || !R || !ks || !workgroups || !to_geom(g, &r)) return 0;
    if (dgrad && !niti::rowconv_dgrad_geom(r, &d)) return 0;
    return niti::rowconv_plan(dgrad ? d : r, dgrad != 0, false, W, R, ks, workgroups) ? 1 : 0;
}

int niti_conv_rows_plan2(const niti_geom* g, int dgrad, int pooled, int* W, int* R, int* ks, int* workgroups) {
    niti::ConvGeom r, d;
    if (!g || !W || !R || !ks || !workgroups || !to_geom(g, &r)) return 0;
    if (dgrad && !niti::rowconv_dgrad_geom(r, &d)) return 0;
    return niti::rowconv_plan(dgrad ? d : r, dgrad != 0, dgrad != 0 && pooled != 0, W, R, ks, workgroups) ? 1 : 0;
}

void niti_diag_rowconv_rows1(int mode) { niti::rowconv_rows1(mode); }

int niti_nhwc16_to_c32(const int8_t* in, int n, int hw, int cp, int c, int8_t* out, void* stream) {
    if (!in || !out || n <= 0 || hw <= 0 || c <= 0 || cp < c || cp % 16) return NITI_INVALID_VALUE;
    return code(niti::nhwc16_to_c32(in, n, hw, cp, c, out, S(stream)));
}

int niti_weights_to_wf(const int8_t* w, int co, int ci, int cip, int transpose, int8_t* out, void* stream) {
    if (!w || !out || co <= 0 || ci <= 0 || cip < ci || cip % 16) return NITI_INVALID_VALUE;
    return code(niti::weights_to_wf(w, co, ci, cip, transpose != 0, out, S(stream)));
}

int niti_conv_rows_nhwc_ok(const niti_geom* g, int dgrad) {
    if (!g) return 0;
    niti::ConvGeom r, d;
    if (!to_geom(g, &r)) return 0;
    const bool pd = dgrad & 2;  // bit 1: whether the model prefers it (not just whether it can)
    if (!(dgrad & 1)) return (pd ? niti::rowconv_nhwc_pref(r) : niti::rowconv_nhwc_ok(r)) ? 1 : 0;
    if (!niti::rowconv_dgrad_geom(r, &d)) return 0;
    return (pd ? niti::rowconv_nhwc_pref(d) : niti::rowconv_nhwc_ok(d)) ? 1 : 0;
}

int niti_conv_fwd_rows(const niti_geom* g, const int8_t* x_c32, const int8_t* wf, const int8_t* exp_in,
                       const int8_t* wscale, int8_t* exp_out, int relu, int8_t* out, int8_t* pool_out,
                       int8_t* next_c32, int mode, uint32_t* amax, uint32_t* state, uint32_t epoch, uint32_t* err,
                       void* stream) {
    const int x_nhwc = (mode & NITI_ROWS_X_NHWC16) ? 1 : 0;
    mode &= ~NITI_ROWS_X_NHWC16;
    if (!g || !x_c32 || !wf || !amax || mode < 0 || mode > 4) return NITI_INVALID_VALUE;
    if (mode >= 3 && state == nullptr) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    if (!niti::rowconv_ok(r)) return NITI_NOT_SUPPORT;
    if (x_nhwc && !niti::rowconv_nhwc_ok(r)) return NITI_NOT_SUPPORT;
    if (mode == 0 && !niti::rowconv_fused_ok(r)) return NITI_NOT_SUPPORT;
    niti::RowConvOut o;
    o.x_nhwc = x_nhwc;
    o.out = out;
    o.pool_out = pool_out;
    o.next = next_c32;
    o.exp_in = exp_in;
    o.wscale = wscale;
    o.exp_out = exp_out;
    o.relu = relu;
    return code(niti::rowconv_fwd(r, x_c32, wf, o, mode, amax, state, epoch, err, S(stream)));
}

int niti_conv_dgrad_rows(const niti_geom* g, const int8_t* dy_c32, const int8_t* wft, const int8_t* relu_mask,
                         const int8_t* pool_x, const int8_t* pool_y, int pool_relu, int8_t* dx, int8_t* dx_c32,
                         int8_t* dx_p16, const int8_t* exp_in, const int8_t* wscale, int8_t* exp_out, int mode,
                         uint32_t* amax, uint32_t* state, uint32_t epoch, uint32_t* err, void* stream) {
    const int x_nhwc = (mode & NITI_ROWS_X_NHWC16) ? 1 : 0;
    mode &= ~NITI_ROWS_X_NHWC16;
    if (!g || !dy_c32 || !wft || !amax || mode < 0 || mode > 4) return NITI_INVALID_VALUE;
    if (mode >= 3 && state == nullptr) return NITI_INVALID_VALUE;
    if ((pool_x == nullptr) != (pool_y == nullptr) || (pool_x && relu_mask)) return NITI_INVALID_VALUE;
    if (mode != 1 && dx == nullptr) return NITI_INVALID_VALUE;
    niti::ConvGeom r, d;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    if (!niti::rowconv_dgrad_geom(r, &d)) return NITI_NOT_SUPPORT;
    if (mode == 0 && !niti::rowconv_fused_ok(d, true, pool_x != nullptr)) return NITI_NOT_SUPPORT;
    if (dx_p16 != nullptr && !niti::rowconv_p16_ok(d, pool_x != nullptr)) return NITI_NOT_SUPPORT;
    if (x_nhwc && !niti::rowconv_nhwc_ok(d)) return NITI_NOT_SUPPORT;
    niti::RowConvOut o;
    o.x_nhwc = x_nhwc;
    o.p16 = dx_p16;
    o.exp_in = exp_in;
    o.wscale = wscale;
    o.exp_out = exp_out;
    o.dgrad_slot = 1;
    if (pool_x != nullptr) {
        o.pool_x = pool_x;
        o.pool_y = pool_y;
        o.pool_dx = dx;
        o.pool_dx_next = dx_c32;
        o.pool_relu = pool_relu;
    } else {
        o.out = dx;
        o.next = dx_c32;
        o.relu_mask = relu_mask;
    }
    return code(niti::rowconv_fwd(d, dy_c32, wft, o, mode, amax, state, epoch, err, S(stream)));
}

int niti_im2col(const niti_geom* g, const int8_t* x, int kp, int8_t* xcol, void* stream) {
    if (!g || !x || !xcol) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    if (r.cip > 16 || r.c_in > 4 || kp % 16 != 0 || kp > 4096 || kp < r.kh * r.kw * r.c_in) return NITI_NOT_SUPPORT;
    return code(niti::im2col_small(r, x, kp, xcol, S(stream)));
}
int niti_im2col_nchw(const niti_geom* g, const int8_t* x_nchw, int kp, int8_t* xcol, void* stream) {
    if (!g || !x_nchw || !xcol) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    if (r.c_in > 4 || kp % 16 != 0 || kp > 4096 || kp < r.kh * r.kw * r.c_in) return NITI_NOT_SUPPORT;
    return code(niti::im2col_small(r, x_nchw, kp, xcol, S(stream), true));
}

int niti_conv_fwd_phase1(const niti_geom* g, const int8_t* x, const int8_t* w, int32_t* acc, uint32_t* amax,
                         void* ws, size_t ws_bytes, void* stream) {
    if (!g || !x || !w || !acc || !amax) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    return code(niti::conv_fwd_phase1(r, x, w, acc, amax, ws, ws ? ws_bytes : 0, S(stream)));
}

int niti_conv_fwd_phase2(const niti_geom* g, const int8_t* x, const int8_t* w, const int32_t* acc,
                         const uint32_t* amax, const int8_t* exp_in, const int8_t* wscale, int8_t* exp_out, int relu,
                         const int8_t* relu_mask, int8_t* out, size_t ws_bytes, void* stream) {
    if (!g || !x || !w || !acc || !amax || !out) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    return code(niti::conv_fwd_phase2(r, x, w, acc, amax, act_out(exp_in, wscale, exp_out, relu, relu_mask, out),
                                      ws_bytes, S(stream)));
}

int niti_conv_dgrad_phase1(const niti_geom* g, const int8_t* dy, const int8_t* wt, int32_t* acc, uint32_t* amax,
                           void* ws, size_t ws_bytes, void* stream) {
    if (!g || !dy || !wt || !acc || !amax) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    return code(niti::conv_dgrad_phase1(r, dy, wt, acc, amax, ws, ws ? ws_bytes : 0, S(stream)));
}

int niti_conv_dgrad_phase2(const niti_geom* g, const int8_t* dy, const int8_t* wt, const int32_t* acc,
                           const uint32_t* amax, const int8_t* exp_in, const int8_t* wscale, int8_t* exp_out, int relu,
                           const int8_t* relu_mask, int8_t* out, size_t ws_bytes, void* stream) {
    if (!g || !dy || !wt || !acc || !amax || !out) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    return code(niti::conv_dgrad_phase2(r, dy, wt, acc, amax, act_out(exp_in, wscale, exp_out, relu, relu_mask, out),
                                        ws_bytes, S(stream)));
}

int niti_conv_wgrad_acc(const niti_geom* g, const int8_t* x, const int8_t* dy, int32_t* acc, uint32_t* amax,
                        void* ws, size_t ws_bytes, void* stream) {
    if (!g) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    return code(niti::conv_wgrad_acc(r, x, dy, acc, amax, ws, ws_bytes, S(stream)));
}

int niti_nhwc16_to_p16(const int8_t* in, int64_t pixels, int cp, int8_t* out, void* stream) {
    if (!in || !out || pixels <= 0 || pixels % 16 || cp <= 0 || cp % 16) return NITI_INVALID_VALUE;
    return code(niti::nhwc16_to_p16(in, pixels, cp, out, S(stream)));
}

void niti_diag_wgrad_stamps(void* buf) { niti::wgrad_stamps_arm((unsigned long long*)buf); }
void niti_diag_rowconv_stamps(void* buf) { niti::rowconv_stamps_arm((unsigned long long*)buf); }
uint32_t* niti_rows_spec_slot(uint32_t* state, int dgrad) {
    return state ? niti::rowconv_spec_slot(state, dgrad != 0) : nullptr;
}

void niti_diag_rowconv_barrier(uint32_t spin_limit, uint32_t expect_extra) {
    niti::rowconv_barrier_diag(spin_limit, expect_extra);
}
void niti_diag_rowconv_speculate(int mode) { niti::rowconv_speculate(mode); }
void niti_diag_gemm_speculate(int bias) { niti::gemm_speculate_bias(bias); }
unsigned long long niti_diag_gemm_fused_launches(void) { return niti::gemm_fused_launches(); }
unsigned long long niti_diag_head_chain_launches(void) { return niti::head_chain_launches(); }
void niti_diag_head_chain(int on) { niti::head_chain_enable(on); }
void niti_diag_p16_jobs_cap(int cap) { niti::model_p16_jobs_cap(cap); }

int niti_conv_wgrad_p16_workspace(const niti_geom* g, int splits, size_t* bytes) {
    if (!g || !bytes) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    if (!niti::conv_wgrad_p16_ok(r)) return NITI_NOT_SUPPORT;
    *bytes = niti::conv_wgrad_p16_workspace(r, splits);
    return NITI_NO_ERROR;
}

int niti_conv_wgrad_p16_acc(const niti_geom* g, const int8_t* x, const int8_t* dy, int32_t* acc, uint32_t* amax,
                            void* ws, size_t ws_bytes, int splits, void* stream) {
    if (!g || !x || !dy || !acc) return NITI_INVALID_VALUE;
    niti::ConvGeom r;
    if (!to_geom(g, &r)) return NITI_COMPUTE_SIZE_ERROR;
    if (!niti::conv_wgrad_p16_ok(r)) return NITI_NOT_SUPPORT;
    if (splits <= 0) splits = niti::conv_wgrad_p16_splits(r);
    if (ws_bytes < niti::conv_wgrad_p16_workspace(r, splits) || (ws_bytes > 0 && !ws)) return NITI_INVALID_VALUE;
    return code(niti::conv_wgrad_p16(r, x, dy, acc, amax, ws, ws_bytes, splits, S(stream)));
}

// the workspace of niti_conv_wgrad_p16_many: the item table (rounded up to 4 KiB), then every job's
// room for 8 slabs
static int p16_many_jobs(const niti_wgrad_p16_job* jobs, int n, int blocks, int t, unsigned char* ws,
                         niti::WgP16Job* out, niti::WgP16Many* m, size_t* table_room, size_t* bytes) {
    if (!jobs || n < 1 || n > niti::P16_MANY_MAX_JOBS || blocks < 1 || t < 1) return NITI_INVALID_VALUE;
    for (int pass = 0; pass < 2; ++pass) {  // the table's size first, then the slabs behind it
        size_t off = *table_room;
        for (int j = 0; j < n; ++j) {
            niti::WgP16Job& o = out[j];
            if (!to_geom(&jobs[j].g, &o.g)) return NITI_COMPUTE_SIZE_ERROR;
            if (!niti::conv_wgrad_p16_ok(o.g)) return NITI_NOT_SUPPORT;
            if (!jobs[j].x_p16 || !jobs[j].dy_p16 || !jobs[j].acc) return NITI_INVALID_VALUE;
            o.x_p16 = jobs[j].x_p16;
            o.dy_p16 = jobs[j].dy_p16;
            o.acc = jobs[j].acc;
            o.amax = jobs[j].amax;
            o.slab_bytes = niti::conv_wgrad_p16_workspace(o.g, 8);
            o.slab = (int32_t*)(ws + off);  // (pass 0: only its being non-null counts)
            off += o.slab_bytes;
        }
        if (niti::conv_wgrad_p16_many_build(out, n, blocks, t, niti::wgrad_quad_kg(niti::P16_QUAD_KG), m) != hipSuccess)
            return NITI_INVALID_VALUE;
        *bytes = off;
        if (pass == 0) *table_room = (m->table_bytes + 4095) / 4096 * 4096;
    }
    return NITI_NO_ERROR;
}

int niti_conv_wgrad_p16_many_workspace(const niti_wgrad_p16_job* jobs, int n, int blocks, int t, size_t* bytes) {
    if (!bytes) return NITI_INVALID_VALUE;
    niti::WgP16Job r[niti::P16_MANY_MAX_JOBS];
    niti::WgP16Many m;
    size_t room = 4096;
    return p16_many_jobs(jobs, n, blocks, t, (unsigned char*)(uintptr_t)4096, r, &m, &room, bytes);
}

int niti_conv_wgrad_p16_many(const niti_wgrad_p16_job* jobs, int n, int blocks, int t, void* ws, size_t ws_bytes,
                             int* splits_out, void* stream) {
    if (!ws) return NITI_INVALID_VALUE;
    niti::WgP16Job r[niti::P16_MANY_MAX_JOBS];
    niti::WgP16Many m;
    size_t room = 4096, need = 0;
    if (const int rc = p16_many_jobs(jobs, n, blocks, t, (unsigned char*)ws, r, &m, &room, &need)) return rc;
    if (ws_bytes < need) return NITI_INVALID_VALUE;
    hipStream_t st = S(stream);
    if (hipMemcpyAsync(ws, m.table, m.table_bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return NITI_NO_EXECUTION;
    hipError_t e = niti::conv_wgrad_p16_many(m, ws, st);
    for (int j = 0; j < n && e == hipSuccess; ++j) {
        if (splits_out) splits_out[j] = m.splits[j];
        if (m.splits[j] > 1)
            e = niti::splitk_reduce_linear(r[j].slab, m.splits[j], (int64_t)r[j].g.c_out * 9 * r[j].g.cip,
                                           m.slab_stride[j], r[j].acc, r[j].amax, st);
    }
    return code(e);
}

// the schedule niti_conv_wgrad_p16_many would run, copied out; no device call (the jobs' pointers
// only have to be non-null)
int niti_conv_wgrad_p16_many_items(const niti_wgrad_p16_job* jobs, int n, int blocks, int t, int* items8,
                                   int cap_items, int* starts, int cap_starts, int* n_items) {
    if (!items8 || !starts || !n_items || cap_items < 0 || cap_starts < 0) return NITI_INVALID_VALUE;
    niti::WgP16Job r[niti::P16_MANY_MAX_JOBS];
    niti::WgP16Many m;
    size_t room = 4096, need = 0;
    if (const int rc = p16_many_jobs(jobs, n, blocks, t, (unsigned char*)(uintptr_t)4096, r, &m, &room, &need)) return rc;
    const int k = niti::conv_wgrad_p16_many_items(m, items8, cap_items, starts, cap_starts);
    if (k < 0) return NITI_INVALID_VALUE;
    *n_items = k;
    return NITI_NO_ERROR;
}

void niti_diag_wgrad_batch(int mode) { niti::model_wgrad_batch(mode); }
void niti_diag_wgrad_quad(int kg) { niti::model_wgrad_quad(kg); }
unsigned long long niti_diag_wgrad_batch_launches(void) { return niti::conv_wgrad_p16_many_launches(); }

int niti_matmul_acc(int m, int o, int k16, const int8_t* B, int64_t ldb, const int8_t* A, int64_t lda, int32_t* acc,
                    int64_t ldc, uint32_t* amax, void* ws, size_t ws_bytes, void* stream) {
    if (k16 % 16 || ldb % 16 || lda % 16 || ldc % 16 || ldc < o) return NITI_INVALID_VALUE;
    return code(niti::matmul_acc(m, o, k16, B, ldb, A, lda, acc, ldc, amax, ws, ws_bytes, S(stream)));
}

int niti_absmax_i32(const int32_t* acc, int64_t n, uint32_t* amax, void* stream) {
    return code(niti::absmax_i32(acc, n, amax, S(stream)));
}

int niti_requant_act(const int32_t* acc, int64_t rows, int ldc, const uint32_t* amax, const int8_t* exp_in,
                     const int8_t* wscale, int8_t* exp_out, int relu, const int8_t* relu_mask, int8_t* out,
                     void* stream) {
    niti::ActRequant r;
    r.acc = acc;
    r.rows = rows;
    r.ldc = ldc;
    r.amax = amax;
    r.exp_in = exp_in;
    r.wscale = wscale;
    r.exp_out = exp_out;
    r.relu = relu;
    r.relu_mask = relu_mask;
    r.out_nhwc16 = out;
    return code(niti::requant_act(r, S(stream)));
}

int niti_requant_act_fused(const int32_t* acc, int64_t rows, int ldc, const uint32_t* amax,
                           const niti_requant_fused* f, void* stream) {
    if (!f || rows < 0) return NITI_INVALID_VALUE;
    niti::ActRequant r;
    r.acc = acc;
    r.rows = rows;
    r.ldc = ldc;
    r.amax = amax;
    r.exp_in = f->exp_in;
    r.wscale = f->wscale;
    r.exp_out = f->exp_out;
    r.relu = f->relu;
    r.relu_mask = f->relu_mask;
    r.out_nhwc16 = f->out_nhwc16;
    r.pool.pool_out = f->pool_out;
    r.pool.x = f->pool_x;
    r.pool.y = f->pool_y;
    r.pool.dx = f->pool_dx;
    r.pool.relu = f->pool_relu;
    r.pool.H = f->pool_h;
    r.pool.W = f->pool_w;
    r.pool.dx_c32 = f->pool_dx_c32;
    r.out_p16 = f->out_p16;
    r.zero_cls = f->zero_cls;
    r.zc_h = f->zc_h;
    r.zc_w = f->zc_w;
    r.pool3.out = f->pool3_out;
    r.pool3.arg = f->pool3_arg;
    r.pool3.H = f->pool3_h;
    r.pool3.W = f->pool3_w;
    r.pool3.OH = f->pool3_oh;
    r.pool3.OW = f->pool3_ow;
    return code(niti::requant_act(r, S(stream)));
}

int niti_requant_grad(const int32_t* acc, int64_t n, const uint32_t* amax, int rule, int8_t* g_out, int8_t* w,
                      void* stream) {
    if (rule != 2 && rule != 3) return NITI_INVALID_VALUE;
    return code(niti::requant_grad(acc, n, amax, rule, g_out, w, S(stream)));
}

int niti_sgd_update(const int32_t* acc, const uint32_t* amax, int rule, int co, int ci, int kk, int cip, int cop,
                    int8_t* w, int8_t* wt, int8_t* g_out, void* stream) {
    if (rule != 2 && rule != 3) return NITI_INVALID_VALUE;
    return code(niti::sgd_update(acc, amax, rule, co, ci, kk, cip, cop, w, wt, g_out, S(stream)));
}
int niti_sgd_update_wf(const int32_t* acc, const uint32_t* amax, int rule, int co, int ci, int kk, int cip, int cop,
                       int8_t* w, int8_t* wt, int8_t* g_out, int8_t* wf, int8_t* wft, void* stream) {
    if (rule != 2 && rule != 3) return NITI_INVALID_VALUE;
    if ((wf || wft) && (kk != 9 || ci % 32 != 0 || co % 32 != 0)) return NITI_NOT_SUPPORT;
    niti::SgdJob j{acc, amax, rule, co, ci, kk, cip, cop, w, wt, g_out};
    j.wf = wf;
    j.wft = wft;
    return code(niti::sgd_update_many(&j, 1, S(stream)));
}

int niti_sgd_combine(const niti_sgd_combine_job* jobs, int n_jobs, void* stream) {
    if (!jobs || n_jobs < 1 || n_jobs > niti::SGD_MAX_JOBS) return NITI_INVALID_VALUE;
    niti::SgdJob r[niti::SGD_MAX_JOBS];
    for (int j = 0; j < n_jobs; ++j) {
        const niti_sgd_combine_job& s = jobs[j];
        if (!s.slab || !s.acc || !s.amax || s.splits < 1 || s.n < 4 || s.n % 4 || s.stride % 4 || s.stride < s.n)
            return NITI_INVALID_VALUE;
        if (((uintptr_t)s.slab | (uintptr_t)s.acc) & 15) return NITI_INVALID_VALUE;
        r[j] = niti::SgdJob{};
        r[j].acc = s.acc;
        r[j].amax = s.amax;
        r[j].slab = s.slab;
        r[j].splits = s.splits;
        r[j].slab_stride = s.stride;
        r[j].slab_n = s.n;
    }
    return code(niti::sgd_combine_many(r, n_jobs, S(stream)));
}

int niti_sgd_update_many(const niti_sgd_job* jobs, int n_jobs, void* stream) {
    if (!jobs || n_jobs < 1 || n_jobs > niti::SGD_MAX_JOBS) return NITI_INVALID_VALUE;
    niti::SgdJob r[niti::SGD_MAX_JOBS];
    for (int j = 0; j < n_jobs; ++j) {
        const niti_sgd_job& s = jobs[j];
        if (!s.acc || !s.amax || !s.w_ohwi16 || (s.rule != 2 && s.rule != 3)) return NITI_INVALID_VALUE;
        if (s.co < 1 || s.ci < 1 || s.kk < 1 || s.cip < s.ci || s.cop < s.co || s.cip % 16 || s.cop % 16)
            return NITI_INVALID_VALUE;
        if ((s.wf || s.wft) && (s.kk != 9 || s.ci % 32 != 0 || s.co % 32 != 0)) return NITI_NOT_SUPPORT;
        r[j] = niti::SgdJob{s.acc, s.amax, s.rule, s.co, s.ci, s.kk, s.cip, s.cop, s.w_ohwi16, s.wt_ihwo16, s.g_out};
        r[j].wf = s.wf;
        r[j].wft = s.wft;
    }
    return code(niti::sgd_update_many(r, n_jobs, S(stream)));
}

int niti_sgd_update_many_bits(const niti_sgd_bits_job* jobs, int n_jobs, const int32_t* bits_dev, void* stream) {
    if (!jobs || !bits_dev || n_jobs < 1 || n_jobs > niti::SGD_MAX_JOBS) return NITI_INVALID_VALUE;
    niti::SgdJob r[niti::SGD_MAX_JOBS];
    for (int j = 0; j < n_jobs; ++j) {
        const niti_sgd_bits_job& b = jobs[j];
        const niti_sgd_job& s = b.job;
        if (!s.acc || !s.amax || !s.w_ohwi16) return NITI_INVALID_VALUE;
        if (s.co < 1 || s.ci < 1 || s.kk < 1 || s.cip < s.ci || s.cop < s.co || s.cip % 16 || s.cop % 16)
            return NITI_INVALID_VALUE;
        if ((s.wf || s.wft) && (s.kk != 9 || s.ci % 32 != 0 || s.co % 32 != 0)) return NITI_NOT_SUPPORT;
        if (b.subw && (b.sub_kh < 1 || b.sub_kw < 1 || b.sub_kh * b.sub_kw != s.kk || b.sub_pt < 0 || b.sub_pl < 0))
            return NITI_INVALID_VALUE;
        if (b.slab && (b.splits < 1 || b.slab_stride % 4 || b.slab_stride < (int64_t)s.co * s.kk * s.cip ||
                       (((uintptr_t)b.slab | (uintptr_t)s.acc) & 15)))
            return NITI_INVALID_VALUE;
        // (the rule field is ignored: job j reads bits_dev[j])
        r[j] = niti::SgdJob{s.acc, s.amax, -(1 + j), s.co, s.ci, s.kk, s.cip, s.cop, s.w_ohwi16, s.wt_ihwo16, s.g_out};
        r[j].wf = s.wf;
        r[j].wft = s.wft;
        if (b.subw) {
            r[j].subw = b.subw;
            r[j].sub_kh = b.sub_kh;
            r[j].sub_kw = b.sub_kw;
            r[j].sub_pt = b.sub_pt;
            r[j].sub_pl = b.sub_pl;
        }
        if (b.slab) {  // C-shaped slabs, summed into acc (and ranged into amax) ahead of the update
            r[j].slab = b.slab;
            r[j].splits = b.splits;
            r[j].slab_stride = b.slab_stride;
            r[j].slab_n = (int64_t)s.co * s.kk * s.cip;
        }
    }
    return code(niti::sgd_update_many(r, n_jobs, S(stream), bits_dev));
}

int niti_input_im2col(const void* in, int quant, int n, int c, int h, int w, int kh, int kw, int pad_t, int pad_l,
                      const uint64_t* stats, int64_t count, int8_t* x_nchw, int8_t* xcol, int8_t* ascale,
                      const int8_t* w0, int co0, int cop0, uint32_t* amax0, void* stream) {
    if (!in || !xcol || n <= 0 || h <= 0 || w <= 0 || pad_t < 0 || pad_l < 0) return NITI_INVALID_VALUE;
    if (!niti::input_im2col_ok(c, kh, kw)) return NITI_NOT_SUPPORT;
    if (quant && (!stats || count <= 0)) return NITI_INVALID_VALUE;
    niti::Conv0Range r0;
    if (w0 != nullptr) {
        r0.w = w0;
        r0.co = co0;
        r0.cop = cop0;
        r0.amax = amax0;
    }
    return code(niti::input_im2col(in, quant != 0, n, c, h, w, kh, kw, pad_t, pad_l,
                                   (const unsigned long long*)stats, quant ? 1 : 0, count, x_nchw, xcol, ascale,
                                   S(stream), r0));
}

int niti_conv0_fwd(const niti_geom* g, const int8_t* xcol, const int8_t* w, uint32_t* amax, const niti_conv0_out* o,
                   int pass, void* stream) {
    niti::ConvGeom r;
    if (!g || !xcol || !w || !amax || !o || pass < 0 || pass > 1 || !to_geom(g, &r)) return NITI_INVALID_VALUE;
    if (!niti::conv0_ok(r)) return NITI_NOT_SUPPORT;
    niti::ActOut a;
    a.out = o->out;
    a.relu = o->relu;
    a.exp_in = o->exp_in;
    a.wscale = o->wscale;
    a.exp_out = o->exp_out;
    a.pool.pool_out = o->pool_out;
    return code(niti::conv0_fwd(r, xcol, w, amax, a, pass, S(stream), o->pool_c32, o->out_c32, o->pool_code));
}
void niti_diag_conv0_blocks(int n) { niti::diag_conv0_blocks(n); }

int niti_conv0_wgrad_codes(int n, int oh, int ow, int cop, int k, const int8_t* g0, const int8_t* code_bytes,
                           const int8_t* xcol, int blocks, int32_t* slab, size_t slab_bytes, int* slabs, void* stream) {
    return code(niti::conv0_wgrad_codes(n, oh, ow, cop, k, g0, code_bytes, xcol, blocks, slab, slab_bytes, slabs,
                                        S(stream)));
}
int niti_conv0_wgrad_codes_slabs(int n, int oh, int ow, int cop, int k, int blocks) {
    return niti::conv0_wgrad_codes_ok(n, oh, ow, cop, k) ? niti::conv0_wgrad_codes_blocks(n, oh, ow, blocks) : 0;
}
void niti_diag_conv0_wgrad_blocks(int n) { niti::diag_conv0_wgrad_blocks(n); }
void niti_diag_conv0_wgrad_codes(int mode) { niti::model_conv0_wgrad_codes(mode); }
unsigned long long niti_diag_conv0_wgrad_codes_launches(void) { return niti::model_conv0_wgrad_codes_launches(); }

// depthwise conv layers (niti_depthwise.hip): every refusal is INVALID_VALUE with nothing launched
static bool dw_geom(const niti_geom* g, niti::ConvGeom* r) { return g != nullptr && to_geom(g, r) && niti::dwconv_ok(*r); }
static niti::ActOut dw_out(const niti_dwconv_out* o) {
    niti::ActOut a;
    a.out = o->out;
    a.relu = o->relu;
    a.relu_mask = o->relu_mask;
    a.exp_in = o->exp_in;
    a.wscale = o->wscale;
    a.exp_out = o->exp_out;
    return a;
}
int niti_dwconv_ok(const niti_geom* g) {
    niti::ConvGeom r;
    return dw_geom(g, &r) ? 1 : 0;
}
int niti_dwconv_fwd(const niti_geom* g, const int8_t* x, const int8_t* w, uint32_t* amax, const niti_dwconv_out* o,
                    int pass, void* stream) {
    niti::ConvGeom r;
    if (!dw_geom(g, &r) || !o) return NITI_INVALID_VALUE;
    return code(niti::dwconv_fwd(r, x, w, amax, dw_out(o), pass, S(stream)));
}
int niti_dwconv_dgrad(const niti_geom* g, const int8_t* dy, const int8_t* w, uint32_t* amax, const niti_dwconv_out* o,
                      int pass, void* stream) {
    niti::ConvGeom r;
    if (!dw_geom(g, &r) || !o) return NITI_INVALID_VALUE;
    return code(niti::dwconv_dgrad(r, dy, w, amax, dw_out(o), pass, S(stream)));
}
int niti_dwconv_wgrad(const niti_geom* g, const int8_t* x, const int8_t* dy, int32_t* slab, size_t slab_bytes,
                      int* slabs, void* stream) {
    niti::ConvGeom r;
    if (!dw_geom(g, &r)) return NITI_INVALID_VALUE;
    return code(niti::dwconv_wgrad(r, x, dy, slab, slab_bytes, slabs, S(stream)));
}
int niti_dwconv_wgrad_slabs(const niti_geom* g) {
    niti::ConvGeom r;
    return dw_geom(g, &r) ? niti::dwconv_wgrad_slabs(r) : 0;
}
int niti_dwconv_wgrad_reduce(const niti_geom* g, const int32_t* slab, int slabs, int32_t* acc, uint32_t* amax,
                             void* stream) {
    niti::ConvGeom r;
    if (!dw_geom(g, &r) || !slab || !acc || slabs != niti::dwconv_wgrad_slabs(r)) return NITI_INVALID_VALUE;
    const int64_t n = (int64_t)r.kh * r.kw * r.cip;
    return code(niti::splitk_reduce_linear(slab, slabs, n, n, acc, amax, S(stream)));
}

// the same at stride 1 or 2 (dwconv2_ok): at stride 1 the launches above
static bool dw2_geom(const niti_geom* g, niti::ConvGeom* r) { return g != nullptr && to_geom(g, r) && niti::dwconv2_ok(*r); }
int niti_dwconv2_ok(const niti_geom* g) {
    niti::ConvGeom r;
    return dw2_geom(g, &r) ? 1 : 0;
}
int niti_dwconv2_fwd(const niti_geom* g, const int8_t* x, const int8_t* w, uint32_t* amax, const niti_dwconv_out* o,
                     int pass, void* stream) {
    niti::ConvGeom r;
    if (!dw2_geom(g, &r) || !o) return NITI_INVALID_VALUE;
    return code(niti::dwconv_fwd(r, x, w, amax, dw_out(o), pass, S(stream)));
}
int niti_dwconv2_dgrad(const niti_geom* g, const int8_t* dy, const int8_t* w, uint32_t* amax, const niti_dwconv_out* o,
                       int pass, void* stream) {
    niti::ConvGeom r;
    if (!dw2_geom(g, &r) || !o) return NITI_INVALID_VALUE;
    return code(niti::dwconv_dgrad(r, dy, w, amax, dw_out(o), pass, S(stream)));
}
int niti_dwconv2_wgrad(const niti_geom* g, const int8_t* x, const int8_t* dy, int32_t* slab, size_t slab_bytes,
                       int* slabs, void* stream) {
    niti::ConvGeom r;
    if (!dw2_geom(g, &r)) return NITI_INVALID_VALUE;
    return code(niti::dwconv_wgrad(r, x, dy, slab, slab_bytes, slabs, S(stream)));
}
int niti_dwconv2_wgrad_slabs(const niti_geom* g) {
    niti::ConvGeom r;
    return dw2_geom(g, &r) ? niti::dwconv_wgrad_slabs(r) : 0;
}
int niti_dwconv2_wgrad_reduce(const niti_geom* g, const int32_t* slab, int slabs, int32_t* acc, uint32_t* amax,
                              void* stream) {
    niti::ConvGeom r;
    if (!dw2_geom(g, &r) || !slab || !acc || slabs != niti::dwconv_wgrad_slabs(r)) return NITI_INVALID_VALUE;
    const int64_t n = (int64_t)r.kh * r.kw * r.cip;
    return code(niti::splitk_reduce_linear(slab, slabs, n, n, acc, amax, S(stream)));
}

int niti_nhwc16_to_chwn16(const int8_t* in, int n, int hw, int cp, int np, int8_t* out, void* stream) {
    return code(niti::nhwc16_to_chwn16(in, n, hw, cp, np, out, S(stream)));
}
int niti_ohwi16_to_ihwo16(const int8_t* w, int co, int ci, int kk, int cip, int cop, int8_t* wt, void* stream) {
    return code(niti::ohwi16_to_ihwo16(w, co, ci, kk, cip, cop, wt, S(stream)));
}
int niti_nchw_to_nhwc16(const int8_t* x, int n, int c, int hw, int cp, int8_t* out, void* stream) {
    return code(niti::nchw_to_nhwc16(x, n, c, hw, cp, out, S(stream)));
}
int niti_nchw_to_chwn16(const int8_t* x, int n, int c, int hw, int cp, int np, int8_t* out, void* stream) {
    return code(niti::nchw_to_chwn16(x, n, c, hw, cp, np, out, S(stream)));
}
int niti_nhwc16_to_nchw(const int8_t* x, int n, int c, int hw, int cp, int8_t* out, void* stream) {
    return code(niti::nhwc16_to_nchw(x, n, c, hw, cp, out, S(stream)));
}
int niti_oihw_to_ohwi16(const int8_t* w, int co, int ci, int kk, int cip, int8_t* out, void* stream) {
    return code(niti::oihw_to_ohwi16(w, co, ci, kk, cip, out, S(stream)));
}
int niti_ohwi16_to_oihw(const int8_t* w, int co, int ci, int kk, int cip, int8_t* out, void* stream) {
    return code(niti::ohwi16_to_oihw(w, co, ci, kk, cip, out, S(stream)));
}
int niti_residual_add(const int8_t* a, const int8_t* ea, const int8_t* b, const int8_t* eb, int64_t n, int32_t* z,
                      int8_t* ez, uint32_t* amax, void* stream) {
    return code(niti::residual_add(a, ea, b, eb, n, z, ez, amax, S(stream)));
}
int niti_residual_requant(const int8_t* a, const int8_t* ea, const int8_t* b, const int8_t* eb, int64_t n,
                          const uint32_t* amax, int8_t* ez, int8_t* exp_out, int relu, int8_t* out, void* stream) {
    return code(niti::residual_requant(a, ea, b, eb, n, amax, ez, exp_out, relu, out, S(stream)));
}
int niti_residual_requant_relu_grad(const int8_t* a, const int8_t* ea, const int8_t* b, const int8_t* eb, int64_t n,
                                    const uint32_t* amax, int8_t* ez, int8_t* exp_out, const int8_t* relu_mask,
                                    int8_t* out, void* stream) {
    if (!relu_mask) return NITI_INVALID_VALUE;
    return code(niti::residual_requant(a, ea, b, eb, n, amax, ez, exp_out, 0, out, S(stream), relu_mask));
}
int niti_sum_pool(const int8_t* x, int n, int hw, int cp, int32_t* acc, uint32_t* amax, void* stream) {
    return code(niti::sum_pool(x, n, hw, cp, acc, amax, S(stream)));
}
int niti_sum_pool_wide(const int8_t* x, int n, int hw, int cp, int32_t* acc, uint32_t* amax, void* stream) {
    return code(niti::sum_pool_wide(x, n, hw, cp, acc, amax, S(stream)));
}
int niti_sum_pool_grad(const int8_t* dy, int n, int hw, int cp, int8_t* dx, void* stream) {
    return code(niti::sum_pool_grad(dy, n, hw, cp, dx, S(stream)));
}
int niti_maxpool(const int8_t* x, int n, int h, int w, int cp, int k, int s, int p, int8_t* y, int oh, int ow,
                 void* stream) {
    return code(niti::maxpool_nhwc16(x, n, h, w, cp, k, s, p, y, oh, ow, S(stream)));
}
int niti_maxpool_grad(const int8_t* x, const int8_t* y, const int8_t* dy, int n, int h, int w, int cp, int k, int s,
                      int p, int oh, int ow, int relu, int8_t* dx, void* stream) {
    return code(niti::maxpool_relu_grad_nhwc16(x, y, dy, n, h, w, cp, k, s, p, oh, ow, relu, dx, S(stream)));
}
int niti_maxpool_grad_ws(const int8_t* x, const int8_t* y, const int8_t* dy, int n, int h, int w, int cp, int k,
                         int s, int p, int oh, int ow, int relu, int8_t* ws, int8_t* dx, void* stream) {
    if (!x || !y || !dy || !ws || !dx || n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) return NITI_INVALID_VALUE;
    return code(niti::maxpool_relu_grad_ws(x, y, dy, n, h, w, cp, k, s, p, oh, ow, relu, ws, dx, S(stream)));
}
int niti_maxpool_arg(const int8_t* x, int n, int h, int w, int cp, int k, int s, int p, int8_t* y, int oh, int ow,
                     int8_t* arg, void* stream) {
    return code(niti::maxpool_nhwc16(x, n, h, w, cp, k, s, p, y, oh, ow, S(stream), arg));
}
int niti_maxpool_grad_arg(const int8_t* x, const int8_t* arg, const int8_t* dy, int n, int h, int w, int cp, int k,
                          int s, int p, int oh, int ow, int relu, const int8_t* pooled, int8_t* dx, void* stream) {
    return code(niti::maxpool_relu_grad_arg(x, arg, dy, n, h, w, cp, k, s, p, oh, ow, relu, dx, S(stream), pooled));
}
int niti_relu_grad(const int8_t* x, const int8_t* dy, int64_t n, int8_t* out, void* stream) {
    if (n % 16) return NITI_INVALID_VALUE;
    return code(niti::relu_grad_nhwc16(x, dy, n, out, S(stream)));
}
int niti_image_stats(const uint8_t* images, int64_t n, uint64_t* stats, void* stream) {
    if (!images || !stats || n <= 0) return NITI_INVALID_VALUE;
    return code(niti::image_stats(images, n, reinterpret_cast<unsigned long long*>(stats), S(stream)));
}
int niti_image_quantize(const uint8_t* images, int n, int c, int hw, const uint64_t* stats, int64_t count,
                        int8_t* out_nchw, int8_t* ascale, void* stream) {
    if (!images || !stats || !out_nchw || n <= 0 || c <= 0 || hw <= 0 || count < (int64_t)n * c * hw)
        return NITI_INVALID_VALUE;
    return code(niti::image_quantize(images, n, c, hw, c, reinterpret_cast<const unsigned long long*>(stats), count,
                                     out_nchw, ascale, false, S(stream)));
}
int niti_image_quantize_nhwc16(const uint8_t* images, int n, int c, int hw, int cp, const uint64_t* stats,
                               int64_t count, int8_t* out_nhwc16, int8_t* ascale, void* stream) {
    if (!images || !stats || !out_nhwc16 || n <= 0 || c <= 0 || hw <= 0 || cp < c || cp % 16 ||
        count < (int64_t)n * c * hw)
        return NITI_INVALID_VALUE;
    return code(niti::image_quantize(images, n, c, hw, cp, reinterpret_cast<const unsigned long long*>(stats), count,
                                     out_nhwc16, ascale, true, S(stream)));
}
int niti_loss_grad(const int8_t* logits, int batch, int classes, int ld, const int8_t* ascale, const int32_t* labels,
                   int8_t* out, void* stream) {
    return code(niti::loss_grad(logits, batch, classes, ld, ascale, labels, out, S(stream)));
}
int niti_head_metrics_workspace(int batch, size_t* bytes) {
    if (!bytes || batch <= 0) return NITI_INVALID_VALUE;
    *bytes = niti::head_metrics_workspace(batch);
    return NITI_NO_ERROR;
}
int niti_head_metrics(const int8_t* logits, int batch, int classes, int ld, const int8_t* ascale,
                      const int32_t* labels, int topk, int32_t* pred, double* loss_per_image, niti_eval_totals* totals,
                      void* workspace, size_t workspace_bytes, void* stream) {
    // every argument is checked on the host before any device call
    if (!logits || !ascale || !labels || !totals) return NITI_INVALID_VALUE;
    if (batch <= 0 || classes <= 0 || ld < classes) return NITI_INVALID_VALUE;
    if (classes > 2048) return NITI_NOT_SUPPORT;
    if (topk < 1 || topk > classes) return NITI_INVALID_VALUE;
    if (!workspace || workspace_bytes < niti::head_metrics_workspace(batch)) return NITI_INVALID_VALUE;
    return code(niti::head_metrics(logits, batch, classes, ld, ascale, labels, topk, pred, loss_per_image, totals,
                                   workspace, workspace_bytes, S(stream)));
}

// ---- device-resident dataset
int niti_dataset_create(const uint8_t* images_nchw, const int32_t* labels, int64_t count, int c, int h, int w,
                        niti_dataset_t* out) {
    if (!images_nchw || !labels || !out || count <= 0 || count > INT32_MAX || c <= 0 || h <= 0 || w <= 0 ||
        (int64_t)c * h * w > INT32_MAX)
        return NITI_INVALID_VALUE;
    auto ds = std::make_unique<niti_dataset>();
    const size_t bytes = (size_t)count * c * h * w;
    if (hipMalloc(&ds->data, bytes) != hipSuccess || hipMalloc(&ds->labels, (size_t)count * 4) != hipSuccess) {
        (void)hipGetLastError();
        return NITI_OUT_OF_MEMORY;
    }
    if (hipMemcpy(ds->data, images_nchw, bytes, hipMemcpyDefault) != hipSuccess ||
        hipMemcpy(ds->labels, labels, (size_t)count * 4, hipMemcpyDefault) != hipSuccess)
        return NITI_NO_EXECUTION;
    ds->count = count;
    ds->c = c;
    ds->h = ds->oh = h;
    ds->w = ds->ow = w;
    *out = ds.release();
    return NITI_NO_ERROR;
}

void niti_dataset_destroy(niti_dataset_t ds) {
    if (ds && ds->index) (void)hipDeviceSynchronize();  // (a gather in flight reads the order and the data)
    delete ds;
}

int niti_dataset_order_check(const int32_t* index, const int32_t* xform, int64_t len, int64_t count, int batch,
                             int allow_pad) {
    if (!index || len <= 0 || count <= 0 || batch <= 0 || len % batch != 0) return NITI_INVALID_VALUE;
    for (int64_t i = 0; i < len; ++i) {
        if (index[i] < (allow_pad ? -1 : 0) || index[i] >= count) return NITI_INVALID_VALUE;
        if (xform && ((uint32_t)xform[i] >> 17) != 0) return NITI_INVALID_VALUE;
    }
    return NITI_NO_ERROR;
}

namespace {

// niti_dataset_set_order / _set_order_windows: the order is checked by the caller
int dataset_set_order(niti_dataset_t ds, const int32_t* index_host, const int32_t* xform_host,
                      const int32_t* window_host, int64_t len) {
    // launches enqueued earlier may still read the previous order: one device synchronisation per
    // order, i.e. per epoch
    if (ds->index && hipDeviceSynchronize() != hipSuccess) return NITI_NO_EXECUTION;
    if (len > ds->order_cap) {
        for (void* p : {(void*)ds->index, (void*)ds->xform_buf})
            if (p) (void)hipFree(p);
        ds->index = ds->xform = ds->xform_buf = nullptr;
        ds->order_cap = 0;
        ds->index_host.clear();
        if (hipMalloc(&ds->index, (size_t)len * 4) != hipSuccess || hipMalloc(&ds->xform_buf, (size_t)len * 4) != hipSuccess) {
            (void)hipGetLastError();
            return NITI_OUT_OF_MEMORY;
        }
        ds->order_cap = len;
    }
    ds->index_host.clear();  // (no order until every copy is in)
    ds->xform = nullptr;
    ds->window = nullptr;
    if (window_host && len > ds->window_cap) {
        if (ds->window_buf) (void)hipFree(ds->window_buf);
        ds->window_buf = nullptr;
        ds->window_cap = 0;
        if (hipMalloc(&ds->window_buf, (size_t)len * 16) != hipSuccess) {
            (void)hipGetLastError();
            return NITI_OUT_OF_MEMORY;
        }
        ds->window_cap = len;
    }
    if (hipMemcpy(ds->index, index_host, (size_t)len * 4, hipMemcpyHostToDevice) != hipSuccess ||
        (xform_host && hipMemcpy(ds->xform_buf, xform_host, (size_t)len * 4, hipMemcpyHostToDevice) != hipSuccess) ||
        (window_host && hipMemcpy(ds->window_buf, window_host, (size_t)len * 16, hipMemcpyHostToDevice) != hipSuccess))
        return NITI_NO_EXECUTION;
    ds->xform = xform_host ? ds->xform_buf : nullptr;
    ds->window = window_host ? ds->window_buf : nullptr;
    ds->index_host.assign(index_host, index_host + len);
    return NITI_NO_ERROR;
}

}  // namespace

int niti_dataset_set_order(niti_dataset_t ds, const int32_t* index_host, const int32_t* xform_host, int64_t len) {
    if (!ds) return NITI_INVALID_VALUE;
    if (const int rc = niti_dataset_order_check(index_host, xform_host, len, ds->count, 1, 1)) return rc;
    return dataset_set_order(ds, index_host, xform_host, nullptr, len);
}

int niti_dataset_set_output(niti_dataset_t ds, int oh, int ow) {
    if (!ds || !niti::resize_size_ok(ds->h, oh) || !niti::resize_size_ok(ds->w, ow) ||
        (int64_t)ds->c * oh * ow > INT32_MAX)
        return NITI_INVALID_VALUE;
    // (a gather in flight was sized by the previous output size and reads the order)
    if (ds->len() > 0 && hipDeviceSynchronize() != hipSuccess) return NITI_NO_EXECUTION;
    ds->index_host.clear();
    ds->xform = nullptr;
    ds->window = nullptr;
    ds->oh = oh;
    ds->ow = ow;
    return NITI_NO_ERROR;
}

int niti_dataset_windows_check(const int32_t* window, const int32_t* xform, int64_t len, int h, int w) {
    if (!window || len <= 0 || h <= 0 || w <= 0) return NITI_INVALID_VALUE;
    for (int64_t i = 0; i < len; ++i) {
        const int64_t x0 = window[4 * i], y0 = window[4 * i + 1], cw = window[4 * i + 2], ch = window[4 * i + 3];
        if (cw < 1 || ch < 1 || x0 < 0 || y0 < 0 || x0 + cw > w || y0 + ch > h) return NITI_INVALID_VALUE;
        if (xform && ((uint32_t)xform[i] & ~(1u << 16)) != 0) return NITI_INVALID_VALUE;
    }
    return NITI_NO_ERROR;
}

int niti_dataset_set_order_windows(niti_dataset_t ds, const int32_t* index_host, const int32_t* xform_host,
                                   const int32_t* window_host, int64_t len) {
    if (!ds) return NITI_INVALID_VALUE;
    if (const int rc = niti_dataset_order_check(index_host, xform_host, len, ds->count, 1, 1)) return rc;
    if (const int rc = niti_dataset_windows_check(window_host, xform_host, len, ds->h, ds->w)) return rc;
    // (a stored size beyond the definition's 32-bit headroom with the default output size)
    if (!niti::resize_size_ok(ds->h, ds->oh) || !niti::resize_size_ok(ds->w, ds->ow)) return NITI_INVALID_VALUE;
    return dataset_set_order(ds, index_host, xform_host, window_host, len);
}

int niti_batch_gather(niti_dataset_t ds, int64_t first, int n, uint8_t* images_out, int32_t* labels_out, void* stream) {
    if (!ds || !images_out || !labels_out || first < 0 || n <= 0 || first > ds->len() - n) return NITI_INVALID_VALUE;
    return code(ds->gather(first, n, images_out, labels_out, S(stream)));
}

}  // extern "C"
