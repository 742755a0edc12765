// niti_internal.hpp -- host-side classes shared by the C ABI translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <vector>

#include "../../include/niti_hip.h"
#include "niti_kernels.hpp"

// A dataset resident in device memory (niti_dataset_*): the images and labels, and the order the
// batch gather (niti_dataset.hip) walks -- on the device, with the index's host copy the step calls
// validate their slice against without a device read.
struct niti_dataset {
    uint8_t* data = nullptr;    // [count][c][h][w]
    int32_t* labels = nullptr;  // [count]
    int64_t count = 0;
    int c = 0, h = 0, w = 0;
    int oh = 0, ow = 0;        // the size of a gathered image (niti_dataset_set_output; default h, w)
    int32_t* index = nullptr;  // [len] (device; capacity order_cap entries)
    int32_t* xform = nullptr;  // [len] or null: no entry is transformed
    int32_t* xform_buf = nullptr;
    int32_t* window = nullptr;  // [len][4] or null: the order has no crop windows
    int32_t* window_buf = nullptr;
    int64_t order_cap = 0, window_cap = 0;
    std::vector<int32_t> index_host;
    int64_t len() const { return (int64_t)index_host.size(); }
    // entries [first, first + n) of the order into out [n][c][oh][ow]: the crop-and-resize gather
    // when the order has windows, else the plain one, which needs oh, ow == h, w
    hipError_t gather(int64_t first, int n, uint8_t* out, int32_t* labels_out, hipStream_t st) const {
        const int32_t* xf = xform ? xform + first : nullptr;
        if (window)
            return niti::batch_gather_resize(data, labels, count, c, h, w, index + first, xf, window + first * 4, n, oh,
                                             ow, out, labels_out, st);
        if (oh != h || ow != w) return hipErrorInvalidValue;
        return niti::batch_gather(data, labels, count, c, h, w, index + first, xf, n, out, labels_out, st);
    }
    ~niti_dataset() {
        for (void* p : {(void*)data, (void*)labels, (void*)index, (void*)xform_buf, (void*)window_buf})
            if (p) (void)hipFree(p);
    }
};

namespace niti {

// Device memory owned by a handle; acquired in onResize, freed on re-resize / destroy
// (the reference acquires DYNAMIC buffers in onResize, NITI_Conv_Int8.cpp:119-157).
struct Workspace {
    std::vector<void*> ptrs;
    size_t total = 0;
    void* alloc(size_t bytes);
    // free `old` (one of ours, or null) and allocate `bytes` in its place
    void* replace(void* old, size_t bytes);
    void release();
    ~Workspace() { release(); }
};

// Execution (execution-engine/source/core/Execution.hpp:24-82) over niti_tensor views.
class Execution {
   public:
    virtual ~Execution() = default;
    virtual int onResize(const niti_tensor* inputs, int nin, const niti_tensor* outputs, int nout) = 0;
    virtual int onExecute(const niti_tensor* inputs, int nin, const niti_tensor* outputs, int nout,
                          hipStream_t st) = 0;
    size_t workspaceBytes() const { return ws_.total; }
    // a device word a launch of this Execution sets when it could not complete (the fused row
    // kernel's grid barrier timed out: results invalid), or null.  niti_execution_execute checks it
    // before a synchronous (host-tensor) call returns, niti_execution_status for device tensors.
    virtual uint32_t* errorFlag() { return nullptr; }

   protected:
    Workspace ws_;
};

Execution* create_execution(int op_type, const niti_conv2d_common* common, int* err);
// CPUTensorConverter::convert for int8 NCHW / NHWC / NC4HW4 (returns an ErrorCode value)
int convert_tensor(const niti_tensor& src, const niti_tensor& dst, hipStream_t st);
bool geom_from_common(const niti_conv2d_common& c, int n, int ci, int h, int w, int co, int kh, int kw,
                      ConvGeom* g);

}  // namespace niti
