/*
 * niti_hip.h -- C ABI of the MI355X (gfx950) NITI int8 training backend.
 *
 * This is the drop-in boundary for the reference's NITI int8 hot path.  The reference
 * exposes that path through MNN's operator interface:
 *
 *   Creator  : CPUBackend::Creator::onCreate(inputs, outputs, const MNN::Op*, Backend*)
 *              execution-engine/source/backend/cpu/CPUBackend.hpp:85-91, registered per
 *              OpType by REGISTER_CPU_OP_CREATOR (:179-182)
 *   Execution: onResize(inputs, outputs) / onExecute(inputs, outputs)
 *              execution-engine/source/core/Execution.hpp:24-82
 *   Errors   : MNN::ErrorCode, execution-engine/include/MNN/ErrorCode.hpp:17-30
 *
 * Section 1 mirrors that interface one to one (niti_create_execution / _resize / _execute /
 * niti_destroy_execution), keyed by the same OpType values, taking the same input and output
 * tensors in the same layouts; an MNN maintainer binds it with a ~40-line Creator (see
 * INTEGRATION.md).  Section 2 is the native split interface the device-resident training
 * driver and data parallelism use (accumulate -> [RCCL] -> requantise).  Section 3 is the
 * whole-step driver (NITIInt8Train's step, execution-engine/tools/train/source/demo/
 * MnistUtils.cpp:68-147, on device) with an optional RCCL communicator.
 *
 * All pointers are device (HBM) pointers unless stated; `stream` is a hipStream_t passed as
 * void*.  No call synchronises the stream or allocates on the execute path.  Handles are not
 * thread safe (as MNN Executions are not re-entrant).
 */
#ifndef NITI_HIP_H
#define NITI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes: MNN::ErrorCode (include/MNN/ErrorCode.hpp:17-30) ------------------------ */
enum niti_error_code {
    NITI_NO_ERROR = 0,
    NITI_OUT_OF_MEMORY = 1,
    NITI_NOT_SUPPORT = 2,
    NITI_COMPUTE_SIZE_ERROR = 3,
    NITI_NO_EXECUTION = 4,
    NITI_INVALID_VALUE = 5,
    NITI_INPUT_DATA_ERROR = 10,
    NITI_CALL_BACK_STOP = 11
};

/* ---- OpType keys (schema/default/MNN.fbs:189-233) ------------------------------------------ */
enum niti_op_type {
    NITI_OP_CONV_INT8 = 700,               /* NITI_CONV_Int8          -> NITI_Conv_Int8.cpp:162-310 */
    NITI_OP_DECONV_INT8 = 701,             /* NITI_DeCONV_Int8        -> NITI_DeConv_Int8.cpp:187-332 */
    NITI_OP_RELU_INT8 = 703,               /* NITI_Relu_Int8          -> NITI_CPURelu_Int8.cpp:28-61 */
    NITI_OP_RELUGRAD_INT8 = 704,           /* NITI_ReluGrad_Int8      -> NITI_CPUReluGrad_Int8.cpp:28-62 */
    NITI_OP_MAXPOOL_INT8 = 705,            /* NITI_Maxpool_Int8       -> NITI_Maxpool_Int8.cpp:24-175 */
    NITI_OP_POOLGRAD_INT8 = 706,           /* NITI_PoolGrad_Int8      -> NITI_CPUPoolGrad_Int8.cpp:21-77 */
    NITI_OP_LOSS_INT8 = 710,               /* NITI_LOSS_Int8          -> NITI_CPULoss_Int8.cpp:68-128 */
    NITI_OP_LOSS_GRAD_INT8 = 711,          /* NITI_LOSS_Grad_Int8     -> NITI_CPULossGrad_Int8.cpp:81-200 */
    NITI_OP_MATMUL_INT8 = 713,             /* NITI_MatMul_Int8        -> NITI_Matmul_Int8.cpp:140-231 */
    NITI_OP_PAD_INT8 = 714,                /* NITI_PAD_Int8           -> NITI_Pad_Int8.cpp:24-62 */
    NITI_OP_GRADIENT_CONV_INT8 = 715,      /* NITI_GradientCONV_Int8  -> NITI_GradientConv_Int8.cpp:165-298 */
    NITI_OP_LEFTPOOLGRAD_INT8 = 718,       /* NITI_LeftPoolGrad_Int8  -> NITI_CPULeftPoolGrad_Int8.cpp:18-52 */
    NITI_OP_DSP_CONV_INT8 = 800,           /* NITI_DSP_CONV_Int8      -> NITI_DSPConv_Int8.cpp:160-455 */
    NITI_OP_DSP_RELU_INT8 = 801,           /* NITI_DSP_RELU_Int8      -> NITI_DSPRelu_Int8.cpp */
    NITI_OP_DSP_MAXPOOL_INT8 = 802,        /* NITI_DSP_MAXPOOL_Int8   -> NITI_DSPMaxpool_Int8.cpp */
    NITI_OP_DSP_RESHAPE_INT8 = 803,        /* NITI_DSP_RESHAPE_Int8   -> NITI_DSPReshape_Int8.cpp */
    NITI_OP_DSP_LOSSGRAD_INT8 = 804,       /* NITI_DSP_LOSSGRAD_Int8  -> NITI_DSPLossGrad_Int8.cpp */
    NITI_OP_DSP_RELUGRAD_INT8 = 805,       /* NITI_DSP_RELUGRAD_Int8  -> NITI_DSPReluGrad_Int8.cpp */
    NITI_OP_DSP_MAXPOOLGRAD_REF_INT8 = 806, /* NITI_DSP_MAXPOOLGRAD_REF_Int8 -> NITI_DSPMaxPoolGradRef_Int8.cpp:17-80 */
    NITI_OP_DSP_MAXPOOLGRAD_INT8 = 807,    /* NITI_DSP_MAXPOOLGRAD_Int8 -> NITI_DSPMaxPoolGrad_Int8.cpp */
    NITI_OP_DSP_TRANSPOSE_INT8 = 808,      /* NITI_DSP_TRANSPOSE_Int8 -> NITI_DSPTranspose_Int8.cpp */
    NITI_OP_DSP_WEIGHTROTATE180_INT8 = 809, /* NITI_DSP_WEIGHTROTATE180_REF_Int8 -> NITI_DSPWeightRotateRef_Int8.cpp */
    NITI_OP_DSP_DECONV_INT8 = 811,         /* NITI_DSP_DECONV_Int8    -> NITI_DSPDeConv_Int8.cpp */
    NITI_OP_DSP_GRADIENTCONV_INT8 = 810,   /* NITI_DSP_GRADIENTCONV_Int8 -> NITI_DSPGradientConv_Int8.cpp (818's tensors) */
    NITI_OP_DSP_PAD_INT8 = 812,            /* NITI_DSP_PAD_Int8       -> NITI_DSPPAD_Int8.cpp */
    NITI_OP_DSP_RESHAPEGRAD_INT8 = 813,    /* NITI_DSP_RESHAPEGrad_Int8 -> NITI_DSPReshapeGrad_Int8.cpp */
    NITI_OP_DSP_LEFTPOOLGRAD_DECONV_INT8 = 814,   /* -> NITI_DSPLeftPoolGrad_Int8.cpp */
    NITI_OP_DSP_LEFTPOOLGRAD_GRADIENT_INT8 = 815, /* -> NITI_DSPLeftPoolGrad_Int8.cpp */
    NITI_OP_DSP_NOP_INT8 = 817,            /* NITI_DSP_NOP_Int8       -> NITI_DSPNop_Int8.cpp */
    NITI_OP_DSP_MATMUL_GRADIENT_INT8 = 818, /* NITI_DSP_MATMUL_GRADIENT_Int8 -> NITI_DSPMatmulGradientConv_Int8.cpp:105-553 */
    NITI_OP_DSP_MATMUL_INT8 = 819,         /* NITI_DSP_MATMUL_Int8    -> NITI_DSPMatmul_Int8.cpp (818's tensors) */
    NITI_OP_DSP_PARALLEL_GRADIENTCONV_INT8 = 820,   /* -> NITI_DSPParallelGradientConv_Int8.cpp (818's tensors) */
    NITI_OP_DSP_GRADIENT_SPLITBATCHCONV_INT8 = 821, /* -> NITI_DSPGradientSplitBatchConv_Int8.cpp (822's tensors) */
    NITI_OP_DSP_TRANSPOSEGRADIENT_CONV_INT8 = 822 /* -> NITI_DSPTransposeGradientConv_Int8.cpp:137-440 */
};

/* ---- tensor formats: MNN_DATA_FORMAT (schema/default/Tensor.fbs:12-18) ---------------------- */
enum niti_format { NITI_FORMAT_NCHW = 0, NITI_FORMAT_NHWC = 1, NITI_FORMAT_NC4HW4 = 2 };

/* ---- pad modes: PadMode (schema/default/CaffeOp.fbs:3-7) ----------------------------------- */
enum niti_pad_mode { NITI_PAD_CAFFE = 0, NITI_PAD_VALID = 1, NITI_PAD_SAME = 2 };

/* A tensor as an Execution sees it: Tensor::host<T>() + batch/channel/height/width +
 * TensorUtils::getDescribe()->dimensionFormat.  dims are the logical N, C, H, W in every
 * format (for NHWC data, dims still list N, C, H, W).  2-D tensors use dims {rows, cols, 1, 1}. */
typedef struct niti_tensor {
    void* data;
    int dims[4];
    int format;
} niti_tensor;

/* The parts of Convolution2DCommon (schema/default/CaffeOp.fbs) the NITI ops read
 * (NeuralNetWorkOp.cpp:1857-1880). pads = {top, left, bottom, right} when has_pads. */
typedef struct niti_conv2d_common {
    int kernel_x, kernel_y;
    int stride_x, stride_y;
    int dilate_x, dilate_y;
    int pad_x, pad_y;
    int has_pads;
    int pads[4];
    int pad_mode;
    int input_count, output_count;
    int group;
} niti_conv2d_common;

/* ============================ 1. Execution-shaped drop-in ============================== */
typedef struct niti_execution* niti_execution_t;

/* CPUBackend::Creator::onCreate for `op_type`.  common may be NULL for NITI_OP_MATMUL_INT8.
 * Returns NITI_NOT_SUPPORT for an op type or parameter the backend does not implement
 * (group != 1; dilation != 1 on a gradient op). */
int niti_create_execution(int op_type, const niti_conv2d_common* common, niti_execution_t* out);

/* Execution::onResize: shape checks + workspace (device memory owned by the handle).
 *  NITI_OP_CONV_INT8          in {x NC4HW4 [N,Ci,H,W], w NCHW [Co,Ci,KH,KW], exp_in int8[1], wscale int8[1]}
 *                             out{y NC4HW4 [N,Co,OH,OW], exp_out int8[1]}
 *  NITI_OP_DECONV_INT8        in {dy' NC4HW4 [N,Co,H',W'] (already padded/dilated by the graph),
 *                                 w^T NCHW [Ci,Co,KH,KW], exp int8[1]}     out{dx NC4HW4 [N,Ci,H,W]}
 *  NITI_OP_GRADIENT_CONV_INT8 in {C4(x^T) NC4HW4 [Ci,N,H,W], dy^T NCHW [Co,N,OH',OW'], ...}
 *                             out{dw NC4HW4 [Ci,Co,KH,KW]}
 *  NITI_OP_MATMUL_INT8        in {B [M,K], A [Co,K]} (2-D, row major)      out{C [M,Co]}
 *  NITI_OP_DSP_MATMUL_GRADIENT_INT8
 *                             in {x NHWC [N,Ci,H,W], dy NHWC [N,Co,OH,OW]} out{dw HWIO [KH,KW,Ci,Co] as
 *                                 dims {KH,KW,Ci,Co}}
 *  NITI_OP_DSP_CONV_INT8, NITI_OP_DSP_DECONV_INT8
 *                             in {x NHWC [N,Ci,H,W], w HWIO as dims {KH,KW,Ci,Co}, exp_in int8[1],
 *                                 wscale int8[1]}                         out{y NHWC [N,Co,OH,OW], exp_out int8[1]}
 *                             (the deconv slot gets the graph's padded/dilated dy and rotated weights)
 *  NITI_OP_DSP_GRADIENTCONV_INT8, NITI_OP_DSP_MATMUL_INT8, NITI_OP_DSP_PARALLEL_GRADIENTCONV_INT8
 *                             as NITI_OP_DSP_MATMUL_GRADIENT_INT8, KH x KW from dw's dims
 *  NITI_OP_RELU_INT8, NITI_OP_RELUGRAD_INT8, NITI_OP_MAXPOOL_INT8, NITI_OP_POOLGRAD_INT8: as the DSP
 *                             slots below, on NC4HW4 (relu / relu grad also NCHW or NHWC) tensors
 *  NITI_OP_DSP_RELU_INT8 / NITI_OP_DSP_NOP_INT8 in {x NHWC} out{y NHWC}; NITI_OP_DSP_RELUGRAD_INT8
 *                             in {x, dy} out{dx}; common may be NULL for these three
 *  NITI_OP_DSP_MAXPOOL_INT8   in {x NHWC, ascale int8[1]} out{y NHWC, ascale int8[1]}; the pool's
 *                             kernel / stride / pad in the common's kernel_x/y, stride_x/y, pad_x/y
 *  NITI_OP_DSP_MAXPOOLGRAD_INT8 in {x, y, dy} NHWC out{dx NHWC}
 *  NITI_OP_DSP_MAXPOOLGRAD_REF_INT8 (806) in {x, y, dy} NHWC out{dx NHWC}: the reference's literal
 *                             walk (x read as [batch][height][width * channel], y / dy at
 *                             (offset * bc) / kernelX / kernelY, untouched bytes kept); kernel /
 *                             stride in the common; NOT_SUPPORT for stride < kernel or windows
 *                             past the tensor (order-dependent / out of bounds in the reference)
 *  NITI_OP_DSP_TRANSPOSE_INT8 in {x, perm int32[4] (device)} out{x permuted}; WEIGHTROTATE180 in {w}
 *                             out{w, raw axes 2, 3 reversed}; RESHAPE / RESHAPEGRAD in {x} out{same bytes};
 *                             all on the stored axis order ([N][H][W][C] for NHWC), common may be NULL
 *  NITI_OP_DSP_PAD_INT8       in {x NHWC} out{NHWC with a zero border of common.pad_x pixels}
 *  NITI_OP_PAD_INT8 (NCHW), NITI_OP_LEFTPOOLGRAD_INT8 (NC4HW4): the CPU graph's pad and stride
 *                             dilation, parameters as the DSP slots'
 *  NITI_OP_DSP_LEFTPOOLGRAD_DECONV_INT8 / _GRADIENT_INT8 in {dy NHWC} out{NHWC, dy[i][j] at
 *                             (stride_y*i, stride_x*j), zeros elsewhere}; stride in the common
 *  NITI_OP_LOSS_GRAD_INT8, NITI_OP_DSP_LOSSGRAD_INT8 (common may be NULL)
 *                             in {logits int8 [batch, classes], ascale int8[1], target int32 one-hot
 *                                 [batch, tc], dy (unused)} out{grad int8 [batch, classes]}; classes <= 2048
 *  NITI_OP_LOSS_INT8 (common may be NULL)
 *                             in {logits int8 [batch, classes], ascale int8[1], target int32 one-hot
 *                                 [batch, tc]} out{loss float32 [1]}: the batch mean of the cross entropy
 *                                 (niti_head_metrics' loss_i, in double; NCHW or NHWC); classes <= 2048
 *  NITI_OP_DSP_TRANSPOSEGRADIENT_CONV_INT8, NITI_OP_DSP_GRADIENT_SPLITBATCHCONV_INT8 (stride 1; the graph
 *                             dilates dy for stride 2)
 *                             in {x^T NHWC [Ci,N,H,W], dy NHWC [N,Co,OH,OW], 0, 0}
 *                             out{dw NHWC [Ci,Co,KH,KW] (kernel size from the shapes), exp_out int8[1] (optional)}
 * Output channel counts must be multiples of 4 on NC4HW4 outputs (the reference sizes its
 * int32 accumulator N*C*H*W but its GEMM writes ceil(C/4)*4 channels): NITI_NOT_SUPPORT. */
int niti_execution_resize(niti_execution_t e, const niti_tensor* inputs, int n_in, const niti_tensor* outputs,
                          int n_out);
/* Execution::onExecute on `stream`: asynchronous for device tensors; with any host tensor it stages
 * them and returns when the host outputs are written, and then also returns NITI_NO_EXECUTION if a
 * launch flagged its results invalid (the fused row kernel's grid barrier timed out: the grid was
 * not resident).  Replaces Execution::onExecute (execution-engine/source/core/Execution.hpp:24-82),
 * codes as ErrorCode.hpp:17-30. */
int niti_execution_execute(niti_execution_t e, const niti_tensor* inputs, int n_in, const niti_tensor* outputs,
                           int n_out, void* stream);
/* the asynchronous path's status: synchronizes `stream`, then NITI_NO_EXECUTION (and the flag
 * cleared) if a launch since the last check flagged invalid results, else NITI_NO_ERROR */
int niti_execution_status(niti_execution_t e, void* stream);
void niti_destroy_execution(niti_execution_t e);
/* bytes of device workspace the handle holds after resize */
size_t niti_execution_workspace_bytes(niti_execution_t e);
/* CPUTensorConverter::convert (source/backend/cpu/CPUTensorConvert.cpp:98-210) for int8 device
 * tensors: NCHW <-> NHWC <-> NC4HW4 (MNN CPU layout [ceil(C/4)][N][H][W][4], pad lanes written as
 * zero).  src and dst have the same logical dims {N, C, H, W}; asynchronous on `stream`.
 * COMPUTE_SIZE_ERROR on a dims mismatch, NOT_SUPPORT on another format, INVALID_VALUE on NULL or
 * in-place buffers. */
int niti_tensor_convert(const niti_tensor* src, const niti_tensor* dst, void* stream);

/* ============================ 2. native split primitives ============================== */
/* A range estimate (max|acc| of one tensor, NITI_RangeEstimate's input, CommonOptFunction.cpp:
 * 1565-1576) is carried in a buffer of NITI_MAX_WORDS uint32 words that the caller zeroes before
 * the producing call.  Producers atomically max into one of 64 slots (one per 128-byte line,
 * word 32*i), spreading the atomics; the value is the max over the slots, which is what every
 * consumer below reads.  An all-reduce (MAX) over the whole buffer of every rank gives the
 * global range in data-parallel exact mode. */
#define NITI_MAX_WORDS 2048
/* Native layouts (padded lanes zero): NHWC16 [N][H][W][round16(C)]; CHWN16 [round16(C)][H][W]
 * [round16(N)]; OHWI16 weights [Co][KH][KW][round16(Ci)]; IHWO16 [Ci][KH][KW][round16(Co)]. */
typedef struct niti_geom {
    int n, c_in, h, w, c_out, kh, kw;
    int stride_h, stride_w, pad_t, pad_l, pad_b, pad_r, dilate_h, dilate_w;
    int oh, ow, cip, cop, np; /* filled by niti_geom_finalize */
} niti_geom;

int niti_geom_finalize(niti_geom* g);

/* Device workspace (bytes) an op needs to split K over workgroups when its output has too
 * few tiles for 256 CUs (op 0 forward, 1 input gradient, 2 weight gradient).  Passing less
 * (or NULL) is allowed: the op then runs unsplit. */
int niti_conv_workspace_bytes(const niti_geom* g, int op, size_t* bytes);
/* The plan a conv GEMM of geometry g runs with under a workspace of ws_bytes (op 0 forward,
 * 1 input gradient, 2 weight gradient): info = {bm, bn, splits, strategy}; bm = bn = 32 is the
 * tap-sharing weight-gradient kernel (stride-1 3x3, Cip % 32 == 0, Cop % 64 == 0). */
int niti_conv_plan_info(const niti_geom* g, int op, size_t ws_bytes, int info[4]);
/* Force the plan a conv GEMM of geometry g runs with (op 0 forward, 1 input gradient, 2 weight
 * gradient; plan as niti_model_plan_set, NULL restores the default); niti_conv_workspace_bytes then
 * reports the workspace the forced plan needs.  Per process, keyed by GEMM shape (what the host-
 * driven ResNet-18 step's autotuner uses). */
int niti_conv_plan_set(const niti_geom* g, int op, const int plan[4]);
int niti_matmul_workspace_bytes(int m, int ldc, int k16, size_t* bytes);
/* acc[n*oh*ow][cop] int32 = conv(x, w); if amax (NITI_MAX_WORDS words): range max-ed in */
int niti_conv_fwd_acc(const niti_geom* g, const int8_t* x_nhwc16, const int8_t* w_ohwi16, int32_t* acc,
                      uint32_t* amax, void* workspace, size_t workspace_bytes, void* stream);
/* acc[n*h*w][cip] int32 = input gradient of the conv for dy (NHWC16) and w^T (IHWO16) */
int niti_conv_dgrad_acc(const niti_geom* g, const int8_t* dy_nhwc16, const int8_t* wt_ihwo16, int32_t* acc,
                        uint32_t* amax, void* workspace, size_t workspace_bytes, void* stream);
/* Two-phase forward / input-gradient conv with the NITI requantisation (NITI_Conv_Int8.cpp:255-307,
 * NITI_DeConv_Int8.cpp:294-329), the training step's path: phase 1 puts max|acc| into amax (zeroed
 * by the caller) -- materialising acc, or, for small K, computing the range only; a data-parallel
 * caller all-reduces amax (MAX) between the phases; phase 2 writes out_nhwc16 = requant(acc) (+ relu,
 * relu_mask as niti_requant_act) and exp_out, recomputing the GEMM where phase 1 stored nothing.
 * acc ([rows][cop] / [rows][cip] int32) and the workspace size must be the same in both calls. */
int niti_conv_fwd_phase1(const niti_geom* g, const int8_t* x_nhwc16, const int8_t* w_ohwi16, int32_t* acc,
                         uint32_t* amax, void* workspace, size_t workspace_bytes, void* stream);
int niti_conv_fwd_phase2(const niti_geom* g, const int8_t* x_nhwc16, const int8_t* w_ohwi16, const int32_t* acc,
                         const uint32_t* amax, const int8_t* exp_in, const int8_t* wscale, int8_t* exp_out, int relu,
                         const int8_t* relu_mask, int8_t* out_nhwc16, size_t workspace_bytes, void* stream);
int niti_conv_dgrad_phase1(const niti_geom* g, const int8_t* dy_nhwc16, const int8_t* wt_ihwo16, int32_t* acc,
                           uint32_t* amax, void* workspace, size_t workspace_bytes, void* stream);
int niti_conv_dgrad_phase2(const niti_geom* g, const int8_t* dy_nhwc16, const int8_t* wt_ihwo16, const int32_t* acc,
                           const uint32_t* amax, const int8_t* exp_in, const int8_t* wscale, int8_t* exp_out,
                           int relu, const int8_t* relu_mask, int8_t* out_nhwc16, size_t workspace_bytes,
                           void* stream);
/* Register-fed forward conv of stride-1 pad-1 3x3 layers with the NITI rescale fused
 * (niti_rowconv.hip; square images of 2, 4, 8 or 16 pixels, c_out padded to 16 a multiple of 32):
 * activations in C32 [n][ceil(C/32)][H][W][32], weights in WF [Co/32][Ci/32][9][2][32][16] (one
 * 1 KiB MFMA fragment per co block, ci block and tap).  mode 0: one launch, max|y| reduced by an
 * in-kernel grid barrier (state: NITI_ROWCONV_STATE_WORDS u32 zeroed once; epoch 1, 2, 3, ... one per
 * call in stream order; err u32 set to 1 if the barrier ever timed out); mode 1: max|y| into amax
 * (zeroed by the caller); mode 2: recompute and requantise with amax (a data-parallel caller
 * all-reduces amax between modes 1 and 2).  Outputs: out_nhwc16 [n][H][W][cop] = relu?(requant(y)),
 * pool_out_nhwc16 (may be NULL) its 2x2 max pool, next_c32 (may be NULL) the (pooled) output as the
 * next layer's C32 input; exp_out = exp_in + wscale + inc.  Modes 3 and 4, the speculative pair
 * (state required; both calls with the same outputs and amax): mode 3 multiplies, requantises with
 * the bit width this state's layer had at its previous mode-4 call and publishes max|y| into amax;
 * mode 4 (after the caller's all-reduce of amax, if any) writes exp_out and redoes the launch only
 * if max|y|'s bit width differs from that guess -- the results are modes 1 + 2's, at one GEMM pass
 * when the bit width holds from step to step. */
#define NITI_ROWCONV_STATE_WORDS 1216
/* the speculative pair's slot of a state (dgrad 0 forward, 1 input gradient): u32 [0] the hint (the
 * bit width on the input's scale: bw + 1 + exp_in + wscale + 512, 0 none), [1] the guess (bw + 1) the
 * last mode-3 call used, [2] the mode-4 calls that redid */
uint32_t* niti_rows_spec_slot(uint32_t* state, int dgrad);
int niti_conv_rows_ok(const niti_geom* g);
/* Which row-kernel instantiation a launch of g runs, by host arithmetic alone (no device call): W the
 * image-row width the kernel is built for (0: the row-segment form), R its output rows per band, ks the
 * channel chunks per wave of the K-split form (0: the general form), workgroups the launch's tiles.
 * g is the LAYER's geometry; dgrad != 0 asks for its input gradient with a fused relu / pool
 * gradient (niti_conv_dgrad_rows).  Returns 1, or 0 where niti_conv_rows_ok refuses the geometry. */
int niti_conv_rows_plan(const niti_geom* g, int dgrad, int* W, int* R, int* ks, int* workgroups);
/* The same with pooled != 0: the input gradient (dgrad != 0) is routed through the previous layer's 2x2
 * max pool (niti_conv_dgrad_rows with pool_x / pool_y).  A pooled 4x4 input gradient whose grid at two
 * rows per band is 384 .. 512 waves runs one row per band (R = 1, twice the workgroups).  pooled = 0 is
 * niti_conv_rows_plan. */
int niti_conv_rows_plan2(const niti_geom* g, int dgrad, int pooled, int* W, int* R, int* ks, int* workgroups);
int niti_nhwc16_to_c32(const int8_t* in_nhwc16, int n, int hw, int cp, int c, int8_t* out_c32, void* stream);
int niti_weights_to_wf(const int8_t* w_ohwi16, int co, int ci, int cip, int transpose, int8_t* out_wf,
                       void* stream);
/* mode | NITI_ROWS_X_NHWC16 (niti_conv_fwd_rows / niti_conv_dgrad_rows): the input (x, or dy) is NHWC16
 * [n][H][W][cip] instead of C32 -- the row-segment maps (niti_conv_rows_nhwc_ok: 14-px multiples
 * above 16 px, or 14 px; cip % 32 == 0) read it in place, with no C32 copy */
#define NITI_ROWS_X_NHWC16 0x100
/* flags bit 0: the input gradient's input (dy) instead of the forward's x; bit 1: whether the
 * library's own step prefers it over a C32 copy (64-channel inputs), not only whether it works */
int niti_conv_rows_nhwc_ok(const niti_geom* g, int flags);
int niti_conv_fwd_rows(const niti_geom* g, const int8_t* x_c32, const int8_t* wf, const int8_t* exp_in,
                       const int8_t* wscale, int8_t* exp_out, int relu, int8_t* out_nhwc16, int8_t* pool_out_nhwc16,
                       int8_t* next_c32, int mode, uint32_t* amax, uint32_t* state, uint32_t epoch, uint32_t* err,
                       void* stream);
/* The input gradient of that conv on the same kernel (NITI_DeConv_Int8.cpp:294-329 with the next
 * op's backward fused): g is the LAYER's geometry; dy_c32 its output gradient in C32, wft the
 * rotated transposed weights (niti_weights_to_wf with transpose = 1); the int32 gradient is
 * requantised by the forward rule (no exponent, no relu) and then either masked by the previous
 * layer's relu (relu_mask NHWC16 [n][H][W][cip]: dx = mask > 0 ? q : 0) into dx_nhwc16, or -- pool_x
 * non-NULL -- routed through the previous layer's 2x2 max pool (pool_x [n][2H][2W][cip] its input,
 * pool_y [n][H][W][cip] its output; pool_relu: zero where pool_x <= 0) into dx_nhwc16 at 2H x 2W.
 * dx_c32 (may be NULL) is the same gradient in C32 (the previous layer's dy_c32), dx_p16 (may be NULL)
 * in the weight gradient's P16 layout [pixels/16][cip][16] (NITI_NOT_SUPPORT where a launch's pixels
 * do not make whole 16-pixel blocks: 4x4 images without the pool at small batches).  exp_out (may be
 * NULL) = exp_in + wscale + the rule's increment, as the forward (NITI_DeConv_Int8 has no exponent
 * output; callers that track gradient exponents, e.g. a residual network, read it here).  mode, amax,
 * state, epoch and err as niti_conv_fwd_rows. */
int niti_conv_dgrad_rows(const niti_geom* g, const int8_t* dy_c32, const int8_t* wft, const int8_t* relu_mask,
                         const int8_t* pool_x, const int8_t* pool_y, int pool_relu, int8_t* dx_nhwc16, int8_t* dx_c32,
                         int8_t* dx_p16, const int8_t* exp_in, const int8_t* wscale, int8_t* exp_out, int mode,
                         uint32_t* amax, uint32_t* state, uint32_t epoch, uint32_t* err, void* stream);
/* acc[co][kh][kw][cip] int32 = weight gradient for x (NHWC16) and dy (NHWC16): a K-major GEMM
 * over the pixels whose operand tiles are transposed in LDS (ds_read_b64_tr_b8) */
int niti_conv_wgrad_acc(const niti_geom* g, const int8_t* x_nhwc16, const int8_t* dy_nhwc16, int32_t* acc,
                        uint32_t* amax, void* workspace, size_t workspace_bytes, void* stream);
/* P16 pixel blocks: an activation of P pixels (P % 16 == 0) and Cp channels as [P/16][Cp][16], so the
 * 16 consecutive pixels of one channel are 16 contiguous bytes -- the MFMA operand fragment of the
 * weight gradient, loaded straight into registers. */
int niti_nhwc16_to_p16(const int8_t* in_nhwc16, int64_t pixels, int cp, int8_t* out_p16, void* stream);
/* Weight gradient on P16 operands (3x3, stride 1, pad 1, Cip % 32 == 0, Cop % 32 == 0, n*oh*ow % 32 == 0,
 * ow in {2, 4, 8, 16} with oh = ow for 2 and 4, oh even for 8):
 * acc[co][kh][kw][cip] int32 (rows < c_out written) and, if amax, its range.  splits <= 0 picks the
 * default.  The workspace holds the split-K partials (niti_conv_wgrad_p16_workspace bytes, 0 without a
 * split).  NOT_SUPPORT for other geometries. */
int niti_conv_wgrad_p16_workspace(const niti_geom* g, int splits, size_t* bytes);
/* diagnostics: device buffer (8 u64 per block) for the per-block stamps of stamp builds; NULL disarms */
void niti_diag_wgrad_stamps(void* buf);
/* diagnostics: device buffer (8 u64 per wave) for the register-fed conv's per-wave stamps; NULL disarms */
void niti_diag_rowconv_stamps(void* buf);
/* diagnostics: the fused row kernel's barrier poll limit (0 = default) and a number of arrivals it
 * waits for that never come (> 0 forces a timeout, to test the error plumbing) for later launches */
void niti_diag_rowconv_barrier(uint32_t spin_limit, uint32_t expect_extra);
/* the fused row kernel's speculative epilogue for later launches: 1 on (the previous launch's bit width
 * is applied while the grid barrier completes, the epilogue redone if it differs), 0 off (default:
 * measured slower), 2 always guess wrong (every launch redoes its epilogue).  Results are identical
 * in every mode. */
void niti_diag_rowconv_speculate(int mode);
/* one row per band for pooled 4x4 input gradients (niti_conv_rows_plan2) for later launches and plans:
 * 1 on, 0 off (two rows per band, as before), -1 the default (on; the environment's NITI_RC_ROWS1=0
 * turns it off).  Results are identical either way.  Set it before a model is created. */
void niti_diag_rowconv_rows1(int mode);
/* diagnostics: launch A of every GEMM speculative pair (plan strategy 3) guesses the layer's previous
 * bit width + bias: +-1 makes launch B settle from an alternate, 2 makes it redo the GEMM (tests);
 * 0 (default) off.  Results are the rule's whatever the bias. */
void niti_diag_gemm_speculate(int bias);
/* diagnostics: implicit-GEMM launches of this process that ran with the rescale fused behind the
 * in-kernel grid barrier (plan strategy 4) */
unsigned long long niti_diag_gemm_fused_launches(void);
/* diagnostics: launches of the classifier head's one-launch chain (forward, loss gradient, weight and
 * input gradient) in this process */
unsigned long long niti_diag_head_chain_launches(void);
/* diagnostics: VGG-11's classifier head as one launch (forward, loss gradient, weight gradient, input
 * gradient through the pool routes; niti_head.hip) instead of four; 0 (default, measured slower) off.
 * Also NITI_HEAD_CHAIN=1.  Results identical either way. */
void niti_diag_head_chain(int on);
/* jobs per P16 input-copy launch of a model step for later steps (<= 0: the default 16); a small
 * cap sends a step down its more-than-one-launch branches.  Results are identical for every cap. */
void niti_diag_p16_jobs_cap(int cap);
int niti_conv_wgrad_p16_acc(const niti_geom* g, const int8_t* x_p16, const int8_t* dy_p16, int32_t* acc,
                            uint32_t* amax, void* workspace, size_t workspace_bytes, int splits, void* stream);
/* Several P16 weight gradients as one persistent launch of `blocks` workgroups: every job is cut into
 * (32 x 32 tile, K range) items of about t K groups (32 pixels each), the items are packed longest
 * first into one list per workgroup, and each workgroup runs its list.  Then acc and, if amax, its
 * range are complete for every job, bit-equal to niti_conv_wgrad_p16_acc (int32 sums are exact).
 * splits_out (may be NULL) receives the number of K ranges each job was cut into.  The workspace
 * (niti_conv_wgrad_p16_many_workspace bytes) holds the item table and the split jobs' partials; the
 * call synchronises the stream once while it uploads the table (the training step keeps its table
 * on the device instead).  At most 16 jobs. */
typedef struct niti_wgrad_p16_job {
    niti_geom g;
    const int8_t* x_p16;
    const int8_t* dy_p16;
    int32_t* acc;
    uint32_t* amax;
} niti_wgrad_p16_job;
int niti_conv_wgrad_p16_many_workspace(const niti_wgrad_p16_job* jobs, int n, int blocks, int t, size_t* bytes);
int niti_conv_wgrad_p16_many(const niti_wgrad_p16_job* jobs, int n, int blocks, int t, void* workspace,
                             size_t workspace_bytes, int* splits_out, void* stream);
/* The training step's 3x3 weight gradients as one such launch after the last input gradient (single
 * device, one stream, at least two P16 layers; a layer with an armed weight-gradient probe keeps its
 * own launch), for models' later steps: 0 off (one launch per layer), 1 (default) the autotuner's
 * choice, which may be off, >= 2 on with items of that many K groups.  Results identical either way. */
void niti_diag_wgrad_batch(int mode);
/* diagnostics: batched weight-gradient launches of this process, captured ones counted once (a
 * graph replay launches without this library) */
unsigned long long niti_diag_wgrad_batch_launches(void);
/* Quad items of that launch: an unsplit job of 2x2 / 4x4 maps whose whole K range is at most kg K
 * groups runs four consecutive tiles per item, one per wave, with no cross-wave sum.  Process-wide:
 * -1 (default) the caller's own threshold (the model's autotuned choice; 32 for
 * niti_conv_wgrad_p16_many), 0 no quad items, kg > 0 that threshold.  Results identical either way. */
void niti_diag_wgrad_quad(int kg);
/* The schedule niti_conv_wgrad_p16_many(jobs, n, blocks, t) would run, copied out without any device
 * call (the jobs' pointers only have to be non-null).  items8: 8 ints per item {job, first tile,
 * tiles of a quad item (0: the merged form, one tile), slab (-1: unsplit), kg_begin, kg_end,
 * kg_per_wave, form (0 merged, 1 quad)}; starts: blocks + 1 list starts (workgroup b runs the items
 * [starts[b], starts[b + 1])).  cap_items / cap_starts: the room, in items and in ints; too little is
 * NITI_INVALID_VALUE. */
int niti_conv_wgrad_p16_many_items(const niti_wgrad_p16_job* jobs, int n, int blocks, int t, int* items8,
                                   int cap_items, int* starts, int cap_starts, int* n_items);
/* acc[m][ldc] = sum_k B[m][k] A[o][k] (columns o..ldc = 0); K zero padded to k16; ldb/lda bytes */
int niti_matmul_acc(int m, int o, int k16, const int8_t* B, int64_t ldb, const int8_t* A, int64_t lda,
                    int32_t* acc, int64_t ldc, uint32_t* amax, void* workspace, size_t workspace_bytes,
                    void* stream);
int niti_absmax_i32(const int32_t* acc, int64_t n, uint32_t* amax, void* stream);
/* forward/deconv rule (NITI_Conv_Int8.cpp:260-307) on acc[rows][ldc]; exp_out = exp_in + wscale + inc
 * (any exponent pointer may be NULL); relu fuses NITI_Relu_Int8; relu_mask (NHWC16) fuses
 * NITI_ReluGrad_Int8.  out_nhwc16 [rows][ldc]. */
int niti_requant_act(const int32_t* acc, int64_t rows, int ldc, const uint32_t* amax, const int8_t* exp_in,
                     const int8_t* wscale, int8_t* exp_out, int relu, const int8_t* relu_mask, int8_t* out_nhwc16,
                     void* stream);
/* The fused forms of the same pass, which the training step (niti_model_*) otherwise reaches alone:
 * the remaining options of the requantisation besides acc, rows, ldc and amax.  Every pointer may be
 * NULL where its form does not need it; the combinations the library cannot run are INVALID_VALUE.
 *  pool_out             forward 2x2 / 2 max pool: rows = pixels [n][pool_h][pool_w] (even sizes); the
 *                       (relu'd) output to out_nhwc16 and its window max to pool_out [n][h/2][w/2][ldc]
 *  pool_dx              its gradient: rows = pooled pixels; each requantised value goes to the first
 *                       max of its window of pool_x (pre-pool output, pooled pool_y) in pool_dx
 *                       [n][pool_h][pool_w][ldc], 0 elsewhere and, with pool_relu, where pool_x <= 0;
 *                       pool_dx_c32 (ldc % 32 == 0): pool_dx also as C32 [n][ldc/32][h][w][32];
 *                       out_nhwc16 (optional) the requantised dy itself
 *  out_p16              the P16 copy [pixels/16][ldc][16] of out_nhwc16 (rows % 16 == 0), or of
 *                       pool_dx (square 2 / 4 / 8 / 16 images, rows a multiple of 4, of 8 at 16)
 *  zero_cls, zc_h, zc_w rows = pixels [n][zc_h][zc_w]: the parity classes (y & 1, x & 1) whose bit
 *                       2 (y & 1) + (x & 1) is set are 0, their accumulators never read (plain pass)
 *  pool3_out, pool3_arg the 3x3 / 2 pad-1 max pool of the output: rows = pixels [n][pool3_h][pool3_w],
 *                       pooled image and first-max positions ky * 3 + kx [n][pool3_oh][pool3_ow][ldc]
 *                       (oh = (h - 1) / 2 + 1); out_nhwc16 optional, no relu_mask */
typedef struct niti_requant_fused {
    const int8_t* exp_in;
    const int8_t* wscale;
    int8_t* exp_out;
    const int8_t* relu_mask;
    int8_t* out_nhwc16;
    int8_t* pool_out;
    const int8_t* pool_x;
    const int8_t* pool_y;
    int8_t* pool_dx;
    int8_t* pool_dx_c32;
    int8_t* out_p16;
    int8_t* pool3_out;
    int8_t* pool3_arg;
    int relu, pool_relu, pool_h, pool_w;
    int zero_cls, zc_h, zc_w;
    int pool3_h, pool3_w, pool3_oh, pool3_ow;
} niti_requant_fused;
int niti_requant_act_fused(const int32_t* acc, int64_t rows, int ldc, const uint32_t* amax,
                           const niti_requant_fused* f, void* stream);
/* gradient rules: rule 2 = NITI_GradientConv_Int8 (bw-2), rule 3 = NITI_Matmul_Int8 (bw-3);
 * g_out optional; w_update optional fused NITI_SGD step w <- clip(w - g, +-127). */
int niti_requant_grad(const int32_t* acc, int64_t n, const uint32_t* amax, int rule, int8_t* g_out,
                      int8_t* w_update, void* stream);
/* Fused NITI_SGD step for one layer: g = rule(acc [co][kk][cip], amax), w <- clip(w - g, +-127)
 * on the OHWI16 weights, the updated weights also written to wt (IHWO16, may be NULL) and g to
 * g_out (OHWI16, may be NULL). */
int niti_sgd_update(const int32_t* acc, const uint32_t* amax, int rule, int co, int ci, int kk, int cip, int cop,
                    int8_t* w_ohwi16, int8_t* wt_ihwo16, int8_t* g_out, void* stream);
/* the same, also rewriting the row kernels' fragment-major copies of a 3x3 layer (niti_weights_to_wf:
 * wf the forward's, wft the input gradient's; either may be NULL; ci, co multiples of 32) in the same
 * pass -- no separate weights_to_wf launches after the update */
int niti_sgd_update_wf(const int32_t* acc, const uint32_t* amax, int rule, int co, int ci, int kk, int cip, int cop,
                       int8_t* w_ohwi16, int8_t* wt_ihwo16, int8_t* g_out, int8_t* wf, int8_t* wft, void* stream);
/* The combine the training step's update launch does first, alone: for every job, acc[i] = the sum
 * over z < splits of slab[z * stride + i] for i < n, and max|acc| into amax (NITI_MAX_WORDS words,
 * zeroed by the caller), all jobs in one launch.  n and stride are multiples of 4, every pointer
 * 16-byte aligned, at most 24 jobs.  A job of few elements over many splits is summed by several
 * lanes per element group; int32 sums are exact in any order. */
typedef struct niti_sgd_combine_job {
    const int32_t* slab;
    int splits;
    int64_t stride;
    int64_t n;
    int32_t* acc;
    uint32_t* amax;
} niti_sgd_combine_job;
int niti_sgd_combine(const niti_sgd_combine_job* jobs, int n_jobs, void* stream);
/* Several layers' NITI_SGD steps in one launch (the training step's update launch; at most 24 jobs):
 * per job niti_sgd_update_wf's arguments.  A workgroup walks tiles of consecutive jobs, each job
 * with its own range and rule. */
typedef struct niti_sgd_job {
    const int32_t* acc;
    const uint32_t* amax;
    int rule, co, ci, kk, cip, cop;
    int8_t* w_ohwi16;
    int8_t* wt_ihwo16;
    int8_t* g_out;
    int8_t* wf;
    int8_t* wft;
} niti_sgd_job;
int niti_sgd_update_many(const niti_sgd_job* jobs, int n_jobs, void* stream);
/* Update bits: the learning rate of a training step, per parameter layer.
 *
 * In NITI the number of bits kept of the int32 weight gradient is the step size.  The reference
 * froze it at 2 (NITI_GradientConv_Int8.cpp:274-296; 3 in its matmul op): rules 2 and 3 above.  A
 * model keeps one int32 word per parameter layer in device memory, `update_bits` in 0..7, 2 from
 * creation; the launches that apply a step's update (the update launch and the fully connected
 * layers' fused update) read the layer's word.  With bw the bit width of the layer's gradient range
 * (NITI_RangeEstimate) and acc its int32 gradient, w <- clip(w - g, +-127) with
 *   bits == 2       exactly rule 2: bw == 0 gives g = 0, else g = PSTO(acc, bw - 2) -- including
 *                   bw == 1, where the shift -1 goes through the reference's PSTO as its x86 build
 *                   executes it.  This negative-shift case deliberately keeps the reference's
 *                   behaviour.
 *   bits 1, 3..7    this library's own extension, as the residual rule is (the reference has no such
 *                   setting): bw == 0 gives g = 0; else sh = bw - bits; sh >= 0 gives
 *                   g = PSTO(acc, sh); sh < 0 gives g = clip(acc, +-127) -- the gradient already
 *                   fits in the bits asked for and is applied as it is.
 *   bits == 0       the layer is frozen: its weights and every derived copy (the transposed, the
 *                   fragment-major and the sub-pixel class weights) are neither changed nor
 *                   rewritten; the kept int8 gradient (niti_model_get_tap which = 1) reads zero.  The
 *                   weight gradient is still computed: no time is saved.
 * The gradient exponent the drop-in DSP Executions report (bw - rule) is no part of a model step
 * and is unchanged.
 *
 * niti_sgd_update_many_bits: the update launch alone under this rule, job k with bits_dev[k] (device
 * memory, n_jobs words, each 0..7); the jobs' rule fields are ignored.  Beside niti_sgd_job's fields a
 * job may carry subw, a stride-2 layer's sub-pixel class weights (the input gradient's layout), with
 * the conv's kernel sub_kh x sub_kw (= kk) and top / left pads, and a deferred split-K combine: slab,
 * `splits` [co][kk][cip] slabs slab_stride elements apart, summed into acc with their range into
 * amax (zeroed by the caller) ahead of the update, as the training step does.  Either may be NULL. */
typedef struct niti_sgd_bits_job {
    niti_sgd_job job;
    int8_t* subw;
    int sub_kh, sub_kw, sub_pt, sub_pl;
    const int32_t* slab;
    int splits;
    int64_t slab_stride;
} niti_sgd_bits_job;
int niti_sgd_update_many_bits(const niti_sgd_bits_job* jobs, int n_jobs, const int32_t* bits_dev, void* stream);
/* The training step's first layer, alone.  niti_input_im2col: the batch (uint8 images quantised
 * with stats = niti_image_stats' four words over `count` pixels when quant, else int8 pixels as
 * they are) into xcol [n * oh * ow][32], the K = 32 im2col copy (stride 1; c / kh / kw = 3/3/3 or
 * 1/5/5), x_nchw (may be NULL) the int8 input, *ascale its exponent (quant only); with w0 (the
 * first conv's weights [co0][32], cop0 = 32 or 64) its range max|y| goes into amax0 as well.
 * niti_conv0_fwd: that conv on xcol (g: 1x1, c_in 32, n / h / w the output's, w % 32 == 0, h even,
 * c_out rounded up to 16 a multiple of 32, else NITI_NOT_SUPPORT): pass 0 the range into amax, pass 1 requantise with
 * it (+ relu) into out (NHWC, may be NULL with pool_out and pool_code) and, with pool_out, the 2x2
 * max pool, its gradient route pool_code and the row kernels' C32 copies (all optional).
 * niti_diag_conv0_blocks: the workgroups of niti_conv0_fwd's launch (0: the default; results do
 * not depend on it). */
int niti_input_im2col(const void* in, int quant, int n, int c, int h, int w, int kh, int kw, int pad_t, int pad_l,
                      const uint64_t* stats, int64_t count, int8_t* x_nchw, int8_t* xcol, int8_t* ascale,
                      const int8_t* w0, int co0, int cop0, uint32_t* amax0, void* stream);
typedef struct niti_conv0_out {
    int8_t* out;
    int8_t* pool_out;
    int8_t* pool_code;
    int8_t* pool_c32;
    int8_t* out_c32;
    const int8_t* exp_in;
    const int8_t* wscale;
    int8_t* exp_out;
    int relu;
} niti_conv0_out;
int niti_conv0_fwd(const niti_geom* g, const int8_t* xcol, const int8_t* w, uint32_t* amax, const niti_conv0_out* o,
                   int pass, void* stream);
void niti_diag_conv0_blocks(int n);
/* The first layer's weight gradient from the pooled gradient and the pool codes, alone.
 * niti_conv0_wgrad_codes: dW0[co][k] = sum over pooled pixels q and window elements t of (g0[q][co]
 * where bit t of code[q][co] is set, else 0) * xcol[pixel t of q's window][k].  g0 and code:
 * [n][oh/2][ow/2][cop] int8 (code: the route bytes niti_conv0_fwd's pool_code holds), xcol
 * [n * oh * ow][32].  The launch leaves *slabs partial sums [cop][32] int32 in slab, cop * 32 elements
 * apart, for niti_sgd_combine (or any sum); niti_conv0_wgrad_codes_slabs is that count, for sizing.
 * blocks: 0 the entry's default, else clamped to the number of 64-pixel steps.  NITI_INVALID_VALUE
 * (nothing launched): oh or ow odd, cop not 32 or 64, k > 32, an operand of 2^31 bytes or more,
 * slab_bytes too small.
 * niti_diag_conv0_wgrad_blocks: the block count the training step passes (0: the default).
 * niti_diag_conv0_wgrad_codes: whether the training step takes this form where it is eligible: -1 the
 * model's own choice (the autotuner's, else the default), 0 off, 1 on (env NITI_CONV0_WGRAD_CODES
 * sets the starting value); niti_diag_conv0_wgrad_codes_launches counts its launches by the step. */
int niti_conv0_wgrad_codes(int n, int oh, int ow, int cop, int k, const int8_t* g0, const int8_t* code,
                           const int8_t* xcol, int blocks, int32_t* slab, size_t slab_bytes, int* slabs, void* stream);
int niti_conv0_wgrad_codes_slabs(int n, int oh, int ow, int cop, int k, int blocks);
void niti_diag_conv0_wgrad_blocks(int n);
void niti_diag_conv0_wgrad_codes(int mode);
unsigned long long niti_diag_conv0_wgrad_codes_launches(void);
/* Depthwise conv layers, alone (csrc/niti_depthwise.hip).  g: c_out == c_in == C, a square 3x3 or 5x5
 * kernel, stride 1, dilation 1, the same pad 0 <= pad < k on every side.  The layer is NITI_Conv_Int8 over
 * the block-diagonal dense weight W[o][i] = (o == i) ? w[o] : 0: forward acc[n][c][oy][ox] = sum over (ky, kx)
 * of x[n][c][oy + ky - pad][ox + kx - pad] w[c][ky][kx] (zero outside the image), its range over the whole
 * tensor, NITI_Conv_Int8's shift rule; the input gradient acc[n][c][y][x] = sum of dy[n][c][y - ky + pad]
 * [x - kx + pad] w[c][ky][kx] under NITI_DeConv_Int8's rule; the weight gradient acc[c][ky][kx] = sum over
 * (n, oy, ox) of dy[n][c][oy][ox] x[n][c][oy + ky - pad][ox + kx - pad], whose range is taken over these
 * C k k values only.  x / dy / out: NHWC16.  w, the int32 gradient and its slabs: [k * k][round16(C)],
 * tap-major -- the OHWI16 form of a c_out = 1, c_in = C layer, whose OIHW host order [1][C][k][k] is the flat
 * order of [C][1][k][k]; niti_sgd_update* and niti_sgd_combine take it as co = 1, ci = C, kk = k * k.
 * niti_dwconv_ok: 1 where the launches take g (host only).
 * niti_dwconv_fwd / _dgrad: pass 0 publishes max|acc| into amax (NITI_MAX_WORDS words, zeroed by the
 *   caller), pass 1 recomputes and requantises with the range found there (a MAX all-reduce may sit between
 *   them); no int32 tensor is written.  relu: forward only; relu_mask (out's shape, out = mask > 0 ? q : 0):
 *   input gradient only.  exp_out = exp_in + wscale + inc (any of the three may be NULL).
 * niti_dwconv_wgrad: leaves *slabs partial sums [k * k][round16(C)] int32 in slab, that many elements
 *   apart; niti_dwconv_wgrad_slabs is the count (a function of g alone; 0 where !niti_dwconv_ok).
 *   niti_dwconv_wgrad_reduce sums them into acc with max|acc| into amax (may be NULL), as the training step
 *   does where the update launch's combine does not.
 * NITI_INVALID_VALUE, nothing launched: a NULL operand, !niti_dwconv_ok(g) (c_in != c_out, k not 3 or 5,
 * stride != 1, an operand of 2^31 bytes or more), pass not 0 / 1, relu with _dgrad or relu_mask with _fwd,
 * slab_bytes too small, slabs != niti_dwconv_wgrad_slabs(g). */
typedef struct niti_dwconv_out {
    int8_t* out;
    const int8_t* relu_mask;
    const int8_t* exp_in;
    const int8_t* wscale;
    int8_t* exp_out;
    int relu;
} niti_dwconv_out;
int niti_dwconv_ok(const niti_geom* g);
int niti_dwconv_fwd(const niti_geom* g, const int8_t* x, const int8_t* w, uint32_t* amax, const niti_dwconv_out* o,
                    int pass, void* stream);
int niti_dwconv_dgrad(const niti_geom* g, const int8_t* dy, const int8_t* w, uint32_t* amax, const niti_dwconv_out* o,
                      int pass, void* stream);
int niti_dwconv_wgrad(const niti_geom* g, const int8_t* x, const int8_t* dy, int32_t* slab, size_t slab_bytes,
                      int* slabs, void* stream);
int niti_dwconv_wgrad_slabs(const niti_geom* g);
int niti_dwconv_wgrad_reduce(const niti_geom* g, const int32_t* slab, int slabs, int32_t* acc, uint32_t* amax,
                             void* stream);
/* The same at stride_h == stride_w == 1 or 2 (the arguments are those of the calls above).  At stride 1 these
 * are the launches above with the same results; at stride 2, with oh = floor((h + 2 pad - k) / 2) + 1 (ow so),
 * the layer is NITI_Conv_Int8 over the same block-diagonal weight with stride 2:
 *   forward          acc[n][c][oy][ox] = sum over (ky, kx) of x[n][c][2 oy + ky - pad][2 ox + kx - pad] w[c][ky][kx]
 *                    (zero outside the image);
 *   input gradient   acc[n][c][y][x] = sum over the (ky, kx) with y + pad - ky and x + pad - kx even and
 *                    oy = (y + pad - ky) / 2, ox = (x + pad - kx) / 2 inside the output of
 *                    dy[n][c][oy][ox] w[c][ky][kx]: each of the four pixel parities has its own tap subset
 *                    (4 / 2 / 2 / 1 taps at 3x3 pad 1, 9 / 6 / 6 / 4 at 5x5 pad 2), and the kernel runs those
 *                    alone, a wave per parity class, reading dy where it lies (no zero-stuffed copy).  Input
 *                    rows and columns no output reads (h + 2 pad - k odd) get 0, written like any other;
 *   weight gradient  acc[c][ky][kx] = sum over (n, oy, ox) of dy[n][c][oy][ox] x[n][c][2 oy + ky - pad][2 ox + kx - pad].
 * Ranges, shift rules, layouts, the two passes and the slabs are as above.  NITI_INVALID_VALUE, nothing
 * launched: everything that is so above, but for stride 2; a stride other than 1 or 2, unequal strides.  The
 * six calls above keep refusing every stride but 1. */
int niti_dwconv2_ok(const niti_geom* g);
int niti_dwconv2_fwd(const niti_geom* g, const int8_t* x, const int8_t* w, uint32_t* amax, const niti_dwconv_out* o,
                     int pass, void* stream);
int niti_dwconv2_dgrad(const niti_geom* g, const int8_t* dy, const int8_t* w, uint32_t* amax, const niti_dwconv_out* o,
                       int pass, void* stream);
int niti_dwconv2_wgrad(const niti_geom* g, const int8_t* x, const int8_t* dy, int32_t* slab, size_t slab_bytes,
                       int* slabs, void* stream);
int niti_dwconv2_wgrad_slabs(const niti_geom* g);
int niti_dwconv2_wgrad_reduce(const niti_geom* g, const int32_t* slab, int slabs, int32_t* acc, uint32_t* amax,
                              void* stream);
/* layout helpers */
int niti_nhwc16_to_chwn16(const int8_t* in, int n, int hw, int cp, int np, int8_t* out, void* stream);
int niti_ohwi16_to_ihwo16(const int8_t* w, int co, int ci, int kk, int cip, int cop, int8_t* wt, void* stream);
int niti_nchw_to_nhwc16(const int8_t* x, int n, int c, int hw, int cp, int8_t* out, void* stream);
int niti_nchw_to_chwn16(const int8_t* x, int n, int c, int hw, int cp, int np, int8_t* out, void* stream);
int niti_nhwc16_to_nchw(const int8_t* x, int n, int c, int hw, int cp, int8_t* out, void* stream);
int niti_oihw_to_ohwi16(const int8_t* w, int co, int ci, int kk, int cip, int8_t* out, void* stream);
int niti_ohwi16_to_oihw(const int8_t* w, int co, int ci, int kk, int cip, int8_t* out, void* stream);
/* rest of the step, NHWC16 */
/* ResNet pieces (niti_resnet.hip; the reference's NITI_Eltwise_Int8 is an empty stub,
 * NITI_Eltwise_Int8.cpp:20-28, so the rule is this library's): z = hi * 2^d + (lo >> r) with
 * d = min(|ea - eb|, 23), r = |ea - eb| - d, hi the operand of the larger exponent (a on ties);
 * *ez = e_hi - d; max|z| into amax.  n % 16 == 0; requantise z with niti_requant_act. */
int niti_residual_add(const int8_t* a, const int8_t* ea, const int8_t* b, const int8_t* eb, int64_t n, int32_t* z,
                      int8_t* ez, uint32_t* amax, void* stream);
/* the fused form: with z = NULL above (range only; a data-parallel caller MAX-reduces amax next),
 * out[n] int8 = the forward rule on z recomputed from a and b (+ relu), exactly as niti_requant_act
 * on the stored z; *ez = e_hi - d and *exp_out = *ez + inc (either may be NULL). */
int niti_residual_requant(const int8_t* a, const int8_t* ea, const int8_t* b, const int8_t* eb, int64_t n,
                          const uint32_t* amax, int8_t* ez, int8_t* exp_out, int relu, int8_t* out, void* stream);
/* the same (no relu), followed by the next op's relu gradient: out = relu_mask > 0 ? q : 0 (the
 * backward residual sum of a block, masked by the previous block's output, NITI_ReluGrad_Int8) */
int niti_residual_requant_relu_grad(const int8_t* a, const int8_t* ea, const int8_t* b, const int8_t* eb, int64_t n,
                                    const uint32_t* amax, int8_t* ez, int8_t* exp_out, const int8_t* relu_mask,
                                    int8_t* out, void* stream);
/* global sum pool: acc[img][c] = sum over hw pixels of x NHWC16 [n][hw][cp] (+ max into amax) */
int niti_sum_pool(const int8_t* x, int n, int hw, int cp, int32_t* acc, uint32_t* amax, void* stream);
/* The same sums and range, for maps of many pixels (a chain network's gpool layer): niti_sum_pool gives
 * each (image, channel) a thread that walks the pixels bytewise, which suits 7x7x512; this one spreads an
 * image's pixels over the lanes of a workgroup, reads 16-byte chunks, keeps a chunk's 16 channels in
 * registers and reduces over the pixel lanes in LDS.  Each sum is written once (no atomics on acc, no
 * int32 tensor beyond acc [n][cp]); max|sum| is MAXed into amax (may be NULL), never stored over it.
 * NITI_INVALID_VALUE, nothing launched: x or acc NULL, n, hw or cp < 1, cp % 16 != 0, hw * 254 >= 2^31,
 * cp > 16 * 16 * 65535 (the channel groups of 16 chunks are a grid dimension). */
int niti_sum_pool_wide(const int8_t* x, int n, int hw, int cp, int32_t* acc, uint32_t* amax, void* stream);
/* its gradient: dx[img][p][c] = dy[img][c] */
int niti_sum_pool_grad(const int8_t* dy, int n, int hw, int cp, int8_t* dx, void* stream);
/* im2col of a shallow NHWC16 input (c_in <= 4; the ResNet-18 stem) for a conv run as a 1x1 conv over
 * kp columns (kp % 16 == 0, kp >= kh * kw * c_in): xcol [n * oh * ow][kp], column k = (ky * kw + kx) *
 * c_in + c, zero beyond kh * kw * c_in and outside the image (the weight [co][kp] in the same order). */
int niti_im2col(const niti_geom* g, const int8_t* x, int kp, int8_t* xcol, void* stream);
/* the same from an int8 NCHW input [n][c_in][h][w] (niti_image_quantize's output) */
int niti_im2col_nchw(const niti_geom* g, const int8_t* x_nchw, int kp, int8_t* xcol, void* stream);
int niti_maxpool(const int8_t* x, int n, int h, int w, int cp, int k, int s, int p, int8_t* y, int oh, int ow,
                 void* stream);
int niti_maxpool_grad(const int8_t* x, const int8_t* y, const int8_t* dy, int n, int h, int w, int cp, int k,
                      int s, int p, int oh, int ow, int relu, int8_t* dx, void* stream);
/* the same gradient in two passes over a caller workspace of n*oh*ow*cp bytes (each window's
 * first-max position, then a gather per input pixel); equal results, for overlapping windows */
int niti_maxpool_grad_ws(const int8_t* x, const int8_t* y, const int8_t* dy, int n, int h, int w, int cp, int k,
                         int s, int p, int oh, int ow, int relu, int8_t* workspace, int8_t* dx, void* stream);
/* niti_maxpool that also records each window's first-max position ky * k + kx (in-image elements
 * in (ky, kx) order) in arg [n][oh][ow][cp]; the training step (ResNet-18's stem) is its other caller.
 * On a map smaller than the kernel y is, as niti_maxpool's, the max of the window clipped to the map
 * size, and arg the first in-image element >= y of the whole window (-1: none), which is where the
 * reference's pool gradient routes. */
int niti_maxpool_arg(const int8_t* x, int n, int h, int w, int cp, int k, int s, int p, int8_t* y, int oh, int ow,
                     int8_t* arg, void* stream);
/* the pool gradient from those positions in one pass: dx = the wrapping int8 sum of dy over the
 * windows whose first max is the pixel; relu masks it by x > 0, or, with pooled (the forward's y; x
 * may then be NULL), each window's term by pooled > 0.  The training step is its other caller. */
int niti_maxpool_grad_arg(const int8_t* x, const int8_t* arg, const int8_t* dy, int n, int h, int w, int cp, int k,
                          int s, int p, int oh, int ow, int relu, const int8_t* pooled, int8_t* dx, void* stream);
int niti_relu_grad(const int8_t* x, const int8_t* dy, int64_t n, int8_t* out, void* stream);
int niti_loss_grad(const int8_t* logits, int batch, int classes, int ld, const int8_t* ascale,
                   const int32_t* labels, int8_t* out, void* stream);
/* Evaluation metrics of a batch of logits (int8 [batch][ld], ld >= classes; lanes classes..ld are
 * padding and never read as classes), what the reference's training program reports: the loss it
 * prints every step (NITI_CPULoss_Int8.cpp:89-125) and the _ArgMax(logits) == label count of its
 * test loop (MnistUtils.cpp:150-181).  Per image i with 0 <= labels[i] < classes:
 *   pred[i]  the first index of the row maximum (a strict > scan, CPUArgMax.cpp:125-130)
 *   rank_i   #{j : l[j] > l[label] or (l[j] == l[label] and j < label)}; top-1 correct <=> rank_i == 0
 *            (<=> pred[i] == label), top-k correct <=> rank_i < topk
 *   loss_i   logsumexp_j(z_j) - z_label with z = l * 2^ascale, evaluated in double (row maximum
 *            subtracted, exact scaling); the reference's float32 MNNSoftmax approximation of the
 *            same value is not reproduced
 * An image with any other label (-1: the padding of a test set's last partial batch) is counted
 * nowhere; its pred is still written and its loss_per_image is 0.  The batch's counts and loss sum
 * are ADDED to *totals (device memory the caller owns and zeroes) in stream order, so a whole test
 * set accumulates without a host synchronisation; the sum runs in a fixed order without atomics
 * (the same inputs give a bit-identical loss_sum).  pred (int32 [batch]) and loss_per_image
 * (double [batch]) may be NULL.  classes <= 2048 (NITI_NOT_SUPPORT above), 1 <= topk <= classes;
 * workspace: niti_head_metrics_workspace(batch) bytes of device memory, 8-byte aligned.  Two
 * launches, asynchronous. */
typedef struct niti_eval_totals {
    uint64_t images, top1, topk;
    double loss_sum;
} niti_eval_totals;
int niti_head_metrics(const int8_t* logits, int batch, int classes, int ld, const int8_t* ascale,
                      const int32_t* labels, int topk, int32_t* pred /*may be NULL*/,
                      double* loss_per_image /*may be NULL*/, niti_eval_totals* totals /*device*/,
                      void* workspace, size_t workspace_bytes, void* stream);
int niti_head_metrics_workspace(int batch, size_t* bytes);

/* NITIInt8Train's input quantiser (execution-engine/tools/train/source/demo/MnistUtils.cpp:83-93):
 * mean / std / range of the uint8 batch, x = round((p - mean) / std / range * 127), ascale =
 * int8(ceilf(logf(range)) - 7) in float.  The variance divisor is the reference's literal
 * batchSize * 28 * 28 (:86), batchSize = count / (c * hw) images, for every image size.  Split so data-parallel ranks can all-reduce the statistics:
 * stats (4 x uint64, device) = {sum p, sum p^2 (SUM over ranks), max p, 255 - min p (MAX)};
 * count = pixels the statistics cover (all ranks').  The float contract (exact integer
 * statistics, the per-pixel formula in the reference's operation order) is stated in
 * csrc/niti_quant.hip.  out_nchw int8 [n][c][hw]; ascale int8 device scalar (may be NULL). */
int niti_image_stats(const uint8_t* images_nchw, int64_t n, uint64_t* stats, void* stream);
int niti_image_quantize(const uint8_t* images_nchw, int n, int c, int hw, const uint64_t* stats, int64_t count,
                        int8_t* out_nchw, int8_t* ascale, void* stream);
/* the same, x written as NHWC16 [n][hw][cp] (cp % 16 == 0, pad channels 0): a conv's input layout */
int niti_image_quantize_nhwc16(const uint8_t* images_nchw, int n, int c, int hw, int cp, const uint64_t* stats,
                               int64_t count, int8_t* out_nhwc16, int8_t* ascale, void* stream);

/* ============================ 3. device-resident training step ========================= */
/* The built-in networks, and any chain of conv / relu / 2x2 max-pool / flatten layers given as a list
 * (niti_chain_layer, niti_model_create_chain below).  LeNet on MNIST 1x28x28 (cfg 1/2); VGG-11 on CIFAR 3x32x32 (cfg 3); VGG-16 on ImageNet 3x224x224
 * with the 4096-4096-1000 head (cfg 4; niti_model_create2 takes another input size, a multiple
 * of 32, e.g. 32 for the oracle-checked tests); ResNet-18 on ImageNet 3x224x224 (cfg 5: 21
 * parameter layers in the order conv1, per basic block conv a / conv b / [1x1 projection], fc; the
 * residual and global-pool rules are this library's -- the reference's NITI_Eltwise_Int8 is a stub,
 * NITI_Eltwise_Int8.cpp:20-28 -- stated in csrc/niti_resnet.hip and oracle/niti_resnet_ref.py), and
 * any residual network of basic blocks given as a stage list (niti_resnet_spec,
 * niti_model_create_resnet below; ResNet-18 is one, and is built through it). */
enum niti_arch { NITI_ARCH_LENET = 1, NITI_ARCH_VGG11 = 2, NITI_ARCH_VGG16 = 3, NITI_ARCH_RESNET18 = 4 };
typedef struct niti_model* niti_model_t;

/* A chain network of the caller's own (niti_model_create_chain): a list of NITI_Conv_Int8 layers,
 * each optionally followed by NITI_Relu_Int8, a 2x2 / stride-2 NITI_Maxpool_Int8 and a flatten, over
 * square in_c x in_hw x in_hw inputs.  Fully connected layers are kernel-1 layers over the 1x1 map a
 * flatten (or the pooling) leaves.  LeNet, VGG-11 and VGG-16 are such lists (csrc/niti_model.hip);
 * a model made from a list reports arch NITI_ARCH_CHAIN, whatever the list. */
enum { NITI_ARCH_CHAIN = 5 };
typedef struct niti_chain_layer {
    int c_out;    /* output channels; the last layer's is the class count */
    int kernel;   /* square kernel size */
    int stride;   /* must be 1 here; 1 or 2 through niti_chain_layer2 and niti_model_chain_check3 / _create_chain3 */
    int pad;      /* symmetric zero padding */
    int relu;     /* NITI_Relu_Int8 after the conv */
    int pool;     /* 2x2 / stride-2 max pool after it (floor, as NITI_Maxpool_Int8) */
    int flatten;  /* the (pooled) output becomes [c*h*w] channels of a 1x1 map, index (c*h + y)*w + x */
} niti_chain_layer;
/* Host only, no device call: validates the list and, if shapes != NULL, writes per layer
 * {c_in, c_out, k, pad, h_in, oh (pre-pool), out_h (after pool / flatten), flat_c (the channels the
 * next layer sees: c_out, or c_out * h * w after a flatten)}.  c_in is derived: in_c for layer 0,
 * else the previous layer's flat_c.
 * NITI_INVALID_VALUE (malformed): layers == NULL, n < 1, in_c < 1, in_hw < 1, and per layer
 *   c_out < 1, kernel < 1, pad < 0, pad >= kernel, a conv output smaller than 1x1
 *   (h + 2 pad < kernel), a pool on a map smaller than 2x2.
 * NITI_NOT_SUPPORT (well formed, not run by this library):
 *   - n > 24: the update launch takes at most that many layers;
 *   - stride != 1 (niti_model_chain_check3 / _create_chain3 below take stride 2);
 *   - kernel > 7: the implicit GEMM's tap loop is generic in the kernel size (above 32 taps the
 *     per-lane loaders serve it); 7 is the largest this library's tests run;
 *   - last layer: c_out > 2048 (the loss and metrics kernels keep a row of logits per thread), a
 *     pool or a flatten, or an output map other than 1x1 (the logits are [batch][classes]);
 *   - a layer after a flatten with kernel != 1 or pad != 0 (its input is a 1x1 map);
 *   - a 3-channel 3x3 or 1-channel 5x5 first layer with 2 pad < kernel (the fused input pass takes
 *     it; with a wider pad the layer runs from the unfused quantiser and is not bound by this) on an
 *     input wider than 32768 / (4 kernel) - kernel + 1 pixels (2728 / 1634): its staged rows would
 *     not fit in LDS;
 *   - any tensor of a layer -- input [b][h][w][c_in up to 32], output [b][oh][ow][c_out up to 16],
 *     flattened output, weights [c_out up to 16][k][k][c_in up to 16] -- above 2^29 elements at batch b
 *     (the GEMM loaders address int8 operands with 31-bit byte offsets and their int32
 *     accumulators are four times the size); niti_model_chain_check tests b = 1,
 *     niti_model_create_chain its own batch.  The products are formed saturating, so sizes past
 *     64 bits are refused like any other.
 * Every list that passes runs: each fast path of the step (csrc/niti_model.hip) is taken per layer
 * by its own shape predicate, with the implicit GEMM + requantise pass and the unfused
 * pool / flatten kernels, which take every shape above, as the fall-back. */
int niti_model_chain_check(const niti_chain_layer* layers, int n, int in_c, int in_hw, int shapes[][8]);
/* The model of a list (batch >= 1).  Runs the check first -- at this batch -- and on a refusal returns
 * its code with nothing allocated and *out untouched.  Every other niti_model_* call takes the
 * handle; niti_model_copy_weights needs the same list and input on both sides. */
int niti_model_create_chain(const niti_chain_layer* layers, int n, int in_c, int in_hw, int batch, niti_model_t* out);
/* The same with depthwise layers (niti_dwconv_* above; this library's extension, stated like the residual
 * rule: the reference's NITI module takes a `depthwise` option, NN.cpp:1118-1125, and its CPU op ignores the
 * group).  niti_chain_layer's seven fields, then depthwise: 1 makes the layer a depthwise conv of its
 * derived c_in channels, weight [C][1][k][k] (niti_model_set_weight / _get_weight / the int8 gradient tap in
 * that order), stride 1.  The two entry points above are these with depthwise = 0 everywhere.  Beside
 * niti_model_chain_check's rule:
 * NITI_INVALID_VALUE (malformed): depthwise other than 0 / 1; a depthwise layer whose c_out is neither 0
 *   ("as the input") nor the derived c_in.
 * NITI_NOT_SUPPORT: a depthwise layer that is layer 0 (the first layer's im2col form), the last layer (the
 *   logits), or that follows a flatten; a depthwise layer with kernel other than 3 or 5.
 * shapes[][8] is niti_model_chain_check's (c_out reported as derived).  A depthwise layer's MACs count
 * n oh ow C k k; niti_model_plan_info / _plan_set on it return NITI_NOT_SUPPORT (it has no GEMM plan) and
 * niti_model_autotune skips it. */
typedef struct niti_chain_layer2 {
    int c_out, kernel, stride, pad, relu, pool, flatten; /* as niti_chain_layer (stride: see niti_model_chain_check3) */
    int depthwise;                                        /* 0: dense; 1: depthwise (c_out 0 or c_in) */
} niti_chain_layer2;
int niti_model_chain_check2(const niti_chain_layer2* layers, int n, int in_c, int in_hw, int shapes[][8]);
int niti_model_create_chain2(const niti_chain_layer2* layers, int n, int in_c, int in_hw, int batch, niti_model_t* out);
/* The same with strided layers: niti_chain_layer2's `stride` is honoured, dense or depthwise (niti_dwconv2_*
 * above), so oh = floor((h + 2 pad - kernel) / stride) + 1.  The four entry points above are these with their
 * refusal of stride != 1 kept.  Beside niti_model_chain_check2's rule:
 * NITI_INVALID_VALUE (malformed): stride < 1.
 * NITI_NOT_SUPPORT: stride > 2; a strided layer after a flatten (its input is a 1x1 map).
 * A strided layer may also pool, may be the first layer and may have kernel 1.  shapes[][8] keeps its meaning
 * (oh under the stride); niti_model_layer_info reports the stride and the MACs count the strided oh ow.  A
 * dense strided layer runs on the implicit GEMM (its input gradient as the sub-pixel class GEMMs on even
 * maps), never in the row or P16 kernels. */
int niti_model_chain_check3(const niti_chain_layer2* layers, int n, int in_c, int in_hw, int shapes[][8]);
int niti_model_create_chain3(const niti_chain_layer2* layers, int n, int in_c, int in_hw, int batch, niti_model_t* out);
/* The same with skip connections, a global sum pool after a layer and up to NITI_CHAIN_MAX_LAYERS layers.
 * niti_chain_layer2's eight fields, then skip and gpool.  The six entry points above are these with
 * skip = gpool = 0 everywhere and their refusals kept: n > 24, and a stride other than 1 where they refuse
 * it.  Both rules are this library's (the reference's NITI_Eltwise_Int8 is a stub), the residual driver's:
 * csrc/niti_resnet.hip, oracle/niti_resnet_ref.py.
 *
 * skip = d >= 1 on layer i: the source is the final output u of layer i - d, after that layer's own add
 * and relu, with its exponent e_u.  The layer's conv runs and is requantised as always, giving y with
 * exponent e_y; then z, e_z = niti_residual_add(y, e_y, u, e_u), the conv output as operand a, and
 * q = the forward rule's requantisation of z (niti_residual_requant; the range MAX-reduced over the ranks
 * in exact data parallelism).  The layer's exponent is e_z + inc; its relu, pool, flatten and gpool follow
 * and apply to q; its relu mask and forward tap are q (y is a temporary).
 *   Backward: every output gradient from the loss back to the earliest source carries its exponent in
 * device memory -- the loss gradient has 0, an input gradient e_dy + wscale + inc, relu, pool, flatten and
 * gpool gradients keep theirs.  dz, the gradient at q after the layer's own relu mask, is the conv's output
 * gradient (weight and input gradient) and, unchanged, the skip's.  At the source s, layer s + 1's input
 * gradient is produced unmasked; niti_residual_add(that gradient, its exponent, dz, e_dz) with the main
 * path as operand a and the requantisation follow, then the source's own relu mask
 * (niti_residual_requant_relu_grad; niti_residual_requant where it has no relu).  The result is the
 * source's output gradient, and its exponent carries on down the chain.
 *   An adding layer and a source run on the implicit GEMM (or the depthwise launches), never in the row
 * kernels or as the head: both operands of a sum are NHWC16.  An adding layer that pools does so after its
 * sum, with the unfused pool kernel; the pool's gradient takes whichever form the next layer's input
 * gradient has for any pooled layer (fused into its requantise pass, or the unfused kernel).
 *
 * gpool = 1: after the layer's relu its oh x ow map is summed per image and channel into
 * int32, the exponent unchanged (niti_sum_pool_wide); the sums are requantised by the forward rule
 * (shift = bitwidth(max|sum|) - 7, exponent e + inc; the range MAX-reduced over the ranks in exact data
 * parallelism).  The output is a 1x1 map of c_out channels, so the next layer has kernel 1 and pad 0, as
 * after a flatten, and shapes[][8] reports out_h = 1 and flat_c = c_out.  The gradient hands the pooled
 * gradient to every pixel of the image, then the layer's relu mask applies (niti_sum_pool_grad).  The
 * layer's forward tap (niti_model_get_tap) stays its (summed) conv + relu output, the map that is pooled.
 *
 * Beside niti_model_chain_check3's rule:
 * NITI_INVALID_VALUE (malformed): gpool other than 0 / 1; skip < 0; i - skip < 0; a source whose output
 *   shape (channels, h, h) is not the adding layer's conv output shape.
 * NITI_NOT_SUPPORT: n > NITI_CHAIN_MAX_LAYERS; gpool together with pool or flatten; gpool on the last
 *   layer; oh * ow * 254 >= 2^31 (the int32 sums); a layer after a gpool layer with kernel != 1 or pad != 0,
 *   a stride other than 1, or depthwise (its input is a 1x1 map); the last layer adds; an adding layer or a
 *   source on the 1x1 map behind a flatten or a gpool; a source that pools, flattens or gpools; a layer that
 *   is the source of two skips; skips whose spans [i - d, i] nest or cross (they may share an endpoint, as
 *   consecutive blocks do).
 * Every list that passes runs.  With 24 layers or fewer the step's launches are those of the same list
 * through the older entry points; past that the update runs in consecutive launches of at most 24 layers. */
#define NITI_CHAIN_MAX_LAYERS 64
typedef struct niti_chain_layer3 {
    int c_out, kernel, stride, pad, relu, pool, flatten, depthwise; /* as niti_chain_layer2 */
    int skip, gpool;                                                /* see above */
} niti_chain_layer3;
int niti_model_chain_check4(const niti_chain_layer3* layers, int n, int in_c, int in_hw, int shapes[][8]);
int niti_model_create_chain4(const niti_chain_layer3* layers, int n, int in_c, int in_hw, int batch, niti_model_t* out);

/* A residual network of the caller's own (niti_model_create_resnet): a stem conv with relu and an
 * optional 3x3 / 2 pad-1 max pool, then n_stages stages of basic blocks, the global sum pool and
 * the fc head, over square in_c x in_hw x in_hw inputs.  ResNet-10 / 18 / 34, narrow or short
 * variants and the CIFAR ResNets (3x3 / 1 stem, no pool, three stages of 16 / 32 / 64) are such
 * specs.  The rule:
 *   - stage s (from 0) has width << s channels and depths[s] basic blocks; conv1 has width;
 *   - a basic block is conv a (3x3, pad 1, relu) and conv b (3x3 / 1, pad 1); conv a has stride 2
 *     on the first block of stages 1 and up, stride 1 elsewhere;
 *   - a block has a 1x1 projection (conv a's stride, pad 0) on its shortcut exactly when its stride
 *     or its channel count differs from its input's; else the shortcut is the block input;
 *   - parameter layers in the order conv1, per block conv a, conv b, [projection], then fc (a 1x1
 *     conv over the global sum pool of the last block: c_in = width << (n_stages - 1));
 *   - the residual sum, the pool and the gradient exponents are ResNet-18's (csrc/niti_resnet.hip,
 *     oracle/niti_resnet_ref.py); without the stem pool block 0 reads relu(conv1) and conv1's output
 *     gradient is the relu gradient of block 0's input gradient.
 * A model made from a spec reports arch NITI_ARCH_RESNET, whatever the spec;
 * niti_model_create3(NITI_ARCH_RESNET18) is the spec {3, 7, 2, 3, 1, 64, 4, {2, 2, 2, 2}, classes}. */
enum { NITI_ARCH_RESNET = 6 };
#define NITI_RESNET_MAX_STAGES 8
/* Parameter layers of a spec model at most.  The caller sizes the check's `shapes` by it; each step
 * updates the layers in ceil(n / 24) launches (at most 11) and keeps three range words and an event
 * per layer.  256 holds every basic-block ResNet in use (ResNet-34: 37, CIFAR ResNet-110: 112,
 * ResNet-1202's 603 is left out on purpose: no test runs past this size). */
#define NITI_RESNET_MAX_LAYERS 256
typedef struct niti_resnet_spec {
    int in_c;                               /* input channels, 1..4 */
    int stem_kernel, stem_stride, stem_pad; /* conv1 (square, symmetric pad), followed by relu */
    int stem_pool;                          /* 1: the 3x3 / 2 pad-1 max pool after it; 0: none */
    int width;                              /* stage s has width << s channels; conv1 has width */
    int n_stages;                           /* 1..NITI_RESNET_MAX_STAGES */
    int depths[NITI_RESNET_MAX_STAGES];     /* basic blocks per stage, each >= 1 (beyond n_stages: ignored) */
    int classes;                            /* <= 2048 */
} niti_resnet_spec;
/* Host only, no device call: validates the spec and writes *n_layers (if not NULL) and, if
 * shapes != NULL, per parameter layer {c_in, c_out, k, stride, pad, h_in, oh, relu} (room for
 * NITI_RESNET_MAX_LAYERS rows is always enough).
 * NITI_INVALID_VALUE (malformed): spec == NULL, in_hw < 1, in_c < 1, stem_kernel < 1,
 *   stem_stride < 1, stem_pad < 0, stem_pad >= stem_kernel, stem_pool other than 0 or 1, width < 1,
 *   n_stages < 1 or > NITI_RESNET_MAX_STAGES, a depth < 1, classes < 1, a stem output below 1x1
 *   (in_hw + 2 stem_pad < stem_kernel; no later layer can drop below 1x1).
 * NITI_NOT_SUPPORT (well formed, not run by this library):
 *   - in_c > 4: the stem's im2col packs a pixel's channels into one dword;
 *   - the stem's im2col columns, stem_kernel^2 in_c rounded up to 32, above 4096 (a thread of the
 *     im2col keeps one 16-byte chunk of a pixel's columns);
 *   - stem_kernel ((ow - 1) stem_stride + stem_kernel) in_c > 16384, ow the stem's output width: the
 *     input rows one output row reads are staged in 16 KiB of LDS;
 *   - classes > 2048 (the loss and metrics kernels keep a row of logits per thread);
 *   - more than NITI_RESNET_MAX_LAYERS parameter layers;
 *   - any tensor -- the input [b][in_c][h][w], a layer's output [b][oh][ow][c_out up to 32], a
 *     layer's input after the stem [b][h][w][c_in up to 32] or weights
 *     [c_out up to 32][k][k][c_in up to 32] -- above 2^29 elements at batch b (31-bit byte offsets,
 *     int32 accumulators of four times the size), or the stem's im2col [b][oh][ow][columns], an int8
 *     operand only, of 2^31 bytes or more; niti_model_resnet_check tests b = 1,
 *     niti_model_create_resnet its own batch.  Products and width << s are formed saturating.
 * Every spec that passes runs, odd map sizes included (a stride-2 conv a and its 1x1 projection
 * agree on them): each layer takes its fast path by its own shape predicate -- stride-1 3x3 layers
 * the register-fed row kernels, stride-2 3x3 input gradients the sub-pixel classes, the rest the
 * implicit GEMM with autotunable plans -- and the implicit GEMM + requantise pass is the fall-back. */
int niti_model_resnet_check(const niti_resnet_spec* spec, int in_hw, int* n_layers, int shapes[][8]);
/* The model of a spec (batch >= 1).  Runs the check first -- at this batch -- and on a refusal returns
 * its code with nothing allocated and *out untouched.  niti_model_copy_weights between two such
 * models needs equal specs and equal in_hw. */
int niti_model_create_resnet(const niti_resnet_spec* spec, int in_hw, int batch, niti_model_t* out);

/* batch = this rank's images per step.  Weights start zero; load them with
 * niti_model_set_weight (OIHW int8, host memory) -- the reference initialises them with a
 * time-seeded RNG (nn/Distributions.cpp:26-51), so callers supply their own. */
int niti_model_create(int arch, int batch, niti_model_t* out);
/* The same with the input resolution (in_hw x in_hw; 0 = the architecture's default). */
int niti_model_create2(int arch, int batch, int in_hw, niti_model_t* out);
/* ... and the class count of the head (0 = the architecture's: 10 LeNet / VGG-11, 1000 VGG-16 /
 * ResNet-18; only ResNet-18 takes another, <= 2048) */
int niti_model_create3(int arch, int batch, int in_hw, int classes, niti_model_t* out);
void niti_model_destroy(niti_model_t m);
int niti_model_num_layers(niti_model_t m);
/* per layer: {c_in, c_out, kh, kw, h_in, w_in, oh, ow, pad, stride, relu, pool} */
int niti_model_layer_info(niti_model_t m, int layer, int info[12]);
/* 1 where the layer is a depthwise conv (niti_chain_layer2), 0 where it is dense, -1 for a NULL handle or
 * a layer out of range */
int niti_model_layer_depthwise(niti_model_t m, int layer);
/* the layer's skip and gpool (niti_chain_layer3; 0 and 0 for every model not made through
 * niti_model_create_chain4); NITI_INVALID_VALUE for a NULL handle or pointer or a layer out of range */
int niti_model_layer_skip(niti_model_t m, int layer, int* skip, int* gpool);
int niti_model_set_weight(niti_model_t m, int layer, const int8_t* w_oihw_host, int wscale);
int niti_model_get_weight(niti_model_t m, int layer, int8_t* w_oihw_host);
/* One NITI_SGD step: forward, NITI_LOSS_Grad, backward, w <- clip(w - g).
 * x: NCHW int8 device [batch][C][H][W]; labels: int32 device [batch]; exp_in: input ascale.
 * Asynchronous on `stream`. */
int niti_model_train_step(niti_model_t m, const int8_t* x_nchw, int exp_in, const int32_t* labels, void* stream);
/* The same step from uint8 images [batch][C][H][W] (device): the input quantiser
 * (niti_image_stats / niti_image_quantize, statistics all-reduced in exact data-parallel mode)
 * runs on device first and supplies x and exp_in -- NITIInt8Train's whole per-batch work. */
int niti_model_train_step_images(niti_model_t m, const uint8_t* images_nchw, const int32_t* labels, void* stream);
/* Forward-only step (evaluation): the training step's forward pass on the current weights -- the
 * logits and their exponent are bit-identical to what niti_model_train_step would have produced
 * from the same weights and input -- followed by niti_head_metrics on the logits, added to the
 * model's running totals.  No weight, derived weight copy, gradient buffer or SGD state is written.
 * Asynchronous, no allocation; always direct launches (the training graph of niti_model_set_graph
 * is neither dropped nor replayed).  labels[i] = -1 excludes image i from the totals (the padding
 * of a last partial batch).  The _images form runs the input quantiser on the batch's own
 * statistics first, as the reference's test loop does (MnistUtils.cpp:161-172).
 * Side effects: niti_model_get_logits, niti_model_get_input and niti_model_get_tap(which = 0) then
 * describe the evaluation batch; taps 1 and 2 still hold the last training step's data;
 * niti_model_rowconv_error covers evaluation launches too.
 * With a communicator or a local group attached the forward issues the same collectives as in
 * training (statistics SUM / MAX, every range MAX in exact mode): world x b evaluates exactly as
 * one device at world * b, all ranks must call it together, and the totals stay rank-local (the
 * caller adds them). */
int niti_model_eval_step(niti_model_t m, const int8_t* x_nchw, int exp_in, const int32_t* labels, void* stream);
int niti_model_eval_step_images(niti_model_t m, const uint8_t* images_nchw, const int32_t* labels, void* stream);
/* the running totals <- 0 (asynchronous) */
int niti_model_eval_reset(niti_model_t m, void* stream);
/* the running totals (synchronises `stream`) */
int niti_model_eval_read(niti_model_t m, niti_eval_totals* host_out, void* stream);
/* the k of the totals' topk count for later evaluation steps (default 5; clamped to [1, classes]) */
int niti_model_eval_topk(niti_model_t m, int k);
/* pred int32 [batch] of the last evaluation batch (synchronises `stream`) */
int niti_model_get_predictions(niti_model_t m, int32_t* pred_host, void* stream);
/* Device-to-device weight hand-over: every layer's weights and weight scale of src into dst on
 * `stream`, dst's derived copies refreshed.  Both models must have the same architecture, input
 * size and class count (hence the same layer shapes; two chain models the same list, two residual
 * models equal specs); the batch may differ -- how a batch-64 training model feeds a batch-20
 * evaluation model.  NITI_INVALID_VALUE otherwise.  Asynchronous. */
int niti_model_copy_weights(niti_model_t dst, niti_model_t src, void* stream);
/* The model's update bits (the rule: "Update bits" at niti_sgd_update_many_bits).
 * niti_model_set_update_bits: layer's word <- bits (layer == -1: every layer), by a kernel on `stream`:
 * asynchronous, in effect for the steps enqueued after it on that stream -- replays of an already
 * captured step (niti_model_set_graph) included, which is neither re-captured nor dropped -- and
 * for the dataset steps of niti_model_train_steps_dataset enqueued after it.  NITI_INVALID_VALUE
 * for bits outside 0..7 or a layer out of range (nothing is written).
 * niti_model_get_update_bits: synchronises `stream` and reads niti_model_num_layers words back.
 * niti_model_copy_weights does not copy the words.  Data parallel: every rank holds its own words
 * and the caller sets them on every rank; ranks that differ are the caller's error and are not
 * detected (the ranks' weights then drift apart). */
int niti_model_set_update_bits(niti_model_t m, int layer, int bits, void* stream);
int niti_model_get_update_bits(niti_model_t m, int32_t* bits_host, void* stream);
/* ---- device-resident dataset ----------------------------------------------------------- */
/* A training or test set kept in device memory, and the batches of an epoch gathered out of it on
 * the device: shuffled, and with the pad-and-crop / horizontal-flip augmentation of CIFAR-class
 * data.  images_nchw uint8 [count][c][h][w] and labels int32 [count] may be host or device
 * pointers; both are copied (synchronously), so the caller's arrays can go.  The images either
 * have the model's input size already, or another size of their own with an output size set
 * (niti_dataset_set_output) and orders that carry crop windows (niti_dataset_set_order_windows). */
typedef struct niti_dataset* niti_dataset_t;
int niti_dataset_create(const uint8_t* images_nchw, const int32_t* labels, int64_t count, int c, int h, int w,
                        niti_dataset_t* out);
/* (synchronises the device when an order was set: a gather in flight reads the dataset) */
void niti_dataset_destroy(niti_dataset_t ds);
/* An order: index[len] (int32: which image each entry is; -1 = a padding entry, a zero image with
 * label -1, as niti_model_eval_step excludes it) and optionally xform[len] (int32), the entry's
 * transform: dx = (int8)(xform & 0xff), dy = (int8)(xform >> 8 & 0xff), flip = xform >> 16 & 1, all
 * 0 without xform.  Entry i with s = index[i] >= 0 is the image
 *   out[ch][y][x] = data[s][ch][y + dy][(flip ? w - 1 - x : x) + dx], 0 where that lies outside
 * -- zero-pad by P, crop at offset (P + dy, P + dx), then mirror; |dx| >= w or |dy| >= h is legal
 * and gives a zero image -- with the label labels[s].  Batch k of an order is its entries
 * [k * batch, (k + 1) * batch).
 * niti_dataset_order_check (host only, no device call) returns NITI_INVALID_VALUE for a NULL index,
 * len <= 0, len % batch != 0, an index outside [-1, count), an index of -1 while allow_pad is 0,
 * and an xform with any bit above 16 set. */
int niti_dataset_order_check(const int32_t* index, const int32_t* xform, int64_t len, int64_t count, int batch,
                             int allow_pad);
/* Checks the order (allow_pad = 1, batch = 1) and copies it to the device (host pointers; xform
 * may be NULL).  Replacing a previous order SYNCHRONISES THE DEVICE first -- steps enqueued earlier
 * may still read it -- which is one synchronisation per epoch.  NITI_NO_EXECUTION if a copy fails
 * (the dataset then has no order).  The order has no crop windows afterwards. */
int niti_dataset_set_order(niti_dataset_t ds, const int32_t* index_host, const int32_t* xform_host, int64_t len);
/* Crop-and-resize: stored images of another size than the model's input.  A dataset has an output
 * size (oh, ow), by default its stored (h, w), and an order may carry, besides index and xform,
 * window[len][4] (int32) = (x0, y0, cw, ch): a rectangle inside the stored image, cw, ch >= 1,
 * x0, y0 >= 0, x0 + cw <= w, y0 + ch <= h.  With windows the xform words may carry the flip bit 16
 * only (dx = dy = 0).  Entry i with s = index[i] >= 0 is its window resized bilinearly, corner
 * pixel to corner pixel, to oh x ow and then mirrored, all in integers (divisions floor):
 *   pos(o, n_out, cn) = 0 if n_out == 1, else (2*o*(cn-1)*256 + (n_out-1)) / (2*(n_out-1))
 *   px = pos(flip ? ow-1-x : x, ow, cw);  ix = x0 + (px >> 8);  fx = px & 255;  ix1 = min(ix+1, x0+cw-1)
 *   py = pos(y, oh, ch);                  iy = y0 + (py >> 8);  fy = py & 255;  iy1 = min(iy+1, y0+ch-1)
 *   A = data[s][c][iy][ix]  B = data[s][c][iy][ix1]  C = data[s][c][iy1][ix]  D = data[s][c][iy1][ix1]
 *   out[i][c][y][x] = (((256-fx)*A + fx*B)*(256-fy) + ((256-fx)*C + fx*D)*fy + 32768) >> 16
 * with the label labels[s]; an index of -1 is a zero image with label -1, as without windows.
 * Positions are rounded to 1/256 px and the weights are exact 8-bit ones, so the result lies within
 * 1.5 of the real-valued bilinear value; a window of exactly ow x oh is the plain crop, a 1x1 window
 * a constant image.  This integer form is the library's own contract (the reference resamples in
 * float).  Every intermediate fits 32 unsigned bits while (ow-1)*(w-1) < 2^22 and
 * (oh-1)*(h-1) < 2^22; sizes beyond that are refused.
 * niti_dataset_set_output: NITI_INVALID_VALUE for a size < 1 or beyond that bound; SYNCHRONISES THE
 * DEVICE if an order is set, and drops the order.
 * niti_dataset_windows_check (host only, no device call): NITI_INVALID_VALUE for a NULL window,
 * len <= 0, h or w <= 0, a window that breaks a rule above, and (xform may be NULL) an xform word
 * with any bit but 16 set.
 * niti_dataset_set_order_windows: niti_dataset_set_order's checks plus the window check, the same
 * synchronise-on-replace rule, NITI_NO_EXECUTION if a copy fails (the dataset then has no order). */
int niti_dataset_set_output(niti_dataset_t ds, int oh, int ow);
int niti_dataset_windows_check(const int32_t* window, const int32_t* xform, int64_t len, int h, int w);
int niti_dataset_set_order_windows(niti_dataset_t ds, const int32_t* index_host, const int32_t* xform_host,
                                   const int32_t* window_host, int64_t len);
/* The primitive: entries [first, first + n) of the order into images_out (uint8 [n][c][h][w],
 * device) and labels_out (int32 [n], device).  One launch, asynchronous, no atomics; nothing outside
 * the dataset is read.  16-byte copies when no xform is set and c*h*w % 16 == 0; with an xform and
 * w % 4 == 0 aligned dword loads, a byte funnel shift and a byte reverse, dword (w % 16 == 0:
 * 16-byte) stores; otherwise a byte per lane.
 * When the order has windows images_out is [n][c][oh][ow] and the crop-and-resize kernel runs: a
 * block builds its entry's column and row positions once (no per-pixel division), a lane produces
 * 16 adjacent pixels and one 16-byte store (ow % 16 == 0, images_out 16-byte aligned), 4 and one
 * dword store (ow % 4 == 0, 4-byte aligned) or one byte; the window words are clamped into the
 * stored image.  Without windows the output size must be the stored size: NITI_INVALID_VALUE
 * otherwise. */
int niti_batch_gather(niti_dataset_t ds, int64_t first, int n, uint8_t* images_out, int32_t* labels_out,
                      void* stream);
/* n_steps training steps, step s (first_step <= s < first_step + n_steps) on batch s of the
 * dataset's order: the batch is gathered into a staging batch the model owns (allocated at the
 * first call), then runs as niti_model_train_step_images does -- the same launches; under
 * niti_model_set_graph(1) one captured step is replayed for every batch, as the staging pointers
 * never change.  Asynchronous: nothing on the host waits, a whole epoch can be enqueued.
 * NITI_INVALID_VALUE, before any launch, for a dataset whose c and output size (oh, ow) are not the
 * model's input, an output size other than the stored size while the order has no windows,
 * first_step / n_steps outside the order, and a -1 entry in the slice.  With a communicator or a
 * local group attached every rank owns its dataset and order (its share of each global batch) and
 * all ranks call together. */
int niti_model_train_steps_dataset(niti_model_t m, niti_dataset_t ds, int64_t first_step, int n_steps, void* stream);
/* The same through niti_model_eval_step_images; -1 entries are allowed (and counted nowhere). */
int niti_model_eval_steps_dataset(niti_model_t m, niti_dataset_t ds, int64_t first_step, int n_steps, void* stream);
/* Training metrics (default 0): when enabled every dataset training step is followed, on the same
 * stream, by niti_head_metrics on the step's logits (what niti_model_get_logits returns after it)
 * and its labels, added to running totals separate from the evaluation's; top-k follows
 * niti_model_eval_topk.  The loss the reference prints every step (NITI_LOSS_Int8), without a
 * synchronisation per step.  Disabled, nothing is launched.  _reset: the totals <- 0
 * (asynchronous); _read synchronises `stream`. */
int niti_model_train_metrics(niti_model_t m, int enable);
int niti_model_train_metrics_reset(niti_model_t m, void* stream);
int niti_model_train_metrics_read(niti_model_t m, niti_eval_totals* host_out, void* stream);
/* Read back (synchronising): the step's quantised input x (NCHW int8) and its exponent. */
int niti_model_get_input(niti_model_t m, int8_t* x_nchw_host, int* ascale, void* stream);
/* Read back (synchronising `stream`): logits [batch][classes] int8 and their exponent. */
int niti_model_get_logits(niti_model_t m, int8_t* logits_host, int* exp_out, void* stream);
/* Per-layer debug taps (synchronising): which = 0 fwd output (post relu, pre pool, NCHW),
 * 1 int8 weight gradient (OIHW), 2 dy of the layer (NCHW, post relu/pool grad). */
int niti_model_get_tap(niti_model_t m, int layer, int which, int8_t* host, size_t bytes, void* stream);
/* Algorithmic int8 MACs per step (unpadded channels; no zero-dilation taps). */
int64_t niti_model_step_macs(niti_model_t m);

/* Keep each step's int8 weight gradient for niti_model_get_tap(which = 1) (default 1).  With 0 the
 * SGD kernel updates the weights from the int32 gradient without storing the int8 copy, and the
 * tap returns NITI_INVALID_VALUE; likewise ResNet-18's stem, whose requantise pass max-pools in
 * the same pass, then writes no pre-pool output (its which = 0 tap returns NITI_INVALID_VALUE). */
int niti_model_keep_grads(niti_model_t m, int enable);
/* Forward convs and input gradients of the stride-1 pad-1 3x3 layers on the register-fed kernel
 * with the rescale fused (niti_rowconv.hip; default 1), or on the LDS-staged GEMM + requantisation
 * passes (0).  Results are identical.  niti_model_rowconv_error: 1 if an in-kernel grid barrier
 * ever timed out (synchronises). */
int niti_model_set_rowconv(niti_model_t m, int enable);
int niti_model_rowconv_error(niti_model_t m);
/* the speculative row-kernel pairs' counters per layer (max_layers x 6 u32): forward hint (bit
 * width + 1), forward launches redone, forward pairs in store mode, then the same for the input
 * gradient (niti_rows_spec_slot; synchronises) */
int niti_model_spec_stats(niti_model_t m, uint32_t* out, int max_layers);
/* diagnostics: the 32 words of one row-kernel layer's speculative slot (niti_rows_spec_slot), with
 * the last 6 pairs' record (bw, input scale, guess) in words 26.. (synchronises) */
int niti_model_spec_slot(niti_model_t m, int layer, int dgrad, uint32_t* out32);
/* Replay the step as a hipGraph (single device only -- with a communicator attached the step
 * always runs as direct launches).  Default 0 (direct launches: measured faster on ROCm 7.2).
 * The captured step holds kernel nodes only (its fills run as kernels: memset nodes were seen to
 * replay wrong values on ROCm 7.2). */
int niti_model_set_graph(niti_model_t m, int enable);
/* Run the weight gradients on a second HIP stream, overlapping the input-gradient chain
 * (default 1; the update waits for both).  With a communicator every collective is still
 * issued on the step stream, in program order, through one communicator. */
int niti_model_set_overlap(niti_model_t m, int enable);
/* Per-shape GEMM plan autotuning (no counterpart in the reference, whose CPU kernels have a
 * fixed blocking, NITI_Conv_Int8.cpp:159-253): times every layer phase under candidate plans
 * (tile shape, store / recompute / split-K count) on `stream` and keeps the fastest for this
 * process.  Plans never change results.  Call after one train_step (it reuses that step's
 * buffers); weights are not touched.  reps <= 0 uses 5.  Synchronises `stream`. */
int niti_model_autotune(niti_model_t m, int reps, void* stream);
/* The plan a layer phase (0 forward, 1 input gradient, 2 weight gradient) runs with:
 * {bm, bn, splits, strategy 0 store / 1 recompute / 2 split-K / 3 the speculative pair (forward and
 * input gradient, unsplit: launch A requantises with the layer's previous bit width and publishes the
 * range, launch B redoes the GEMM only when the range's bit width differs) / 4 fused (forward and
 * stride-1 input gradient, unsplit: one launch whose blocks keep their accumulators in registers
 * across an in-kernel grid barrier carrying the tensor's bit width, then requantise -- where every
 * tile is resident at once and no collective sits between range and requantisation; elsewhere it
 * runs as 1)}. */
int niti_model_plan_info(niti_model_t m, int layer, int phase, int info[4]);
/* Force a plan for a layer phase ({bm 64|128, bn 64|128, splits >= 1, strategy}; split counts
 * beyond the K steps or the workspace are clamped; recompute on the weight gradient means
 * store); plan = NULL restores the default.  Overrides are per process, keyed by GEMM shape. */
int niti_model_plan_set(niti_model_t m, int layer, int phase, const int plan[4]);
/* Drop every plan override of the process (autotuned or forced). */
void niti_plan_reset(void);
/* Kernel probe: HIP events on the step's stream around one GEMM launch (layer, phase
 * 0 = forward, 1 = input gradient, 2 = weight gradient) for up to max_launches steps;
 * layer < 0 disables.  probe_read synchronises those events and returns the summed
 * duration and the number of launches timed, then resets the count. */
int niti_model_set_probe(niti_model_t m, int layer, int phase, int max_launches);
int niti_model_probe_read(niti_model_t m, double* total_ms, int* count);
/* paused != 0: the armed probe skips the next launches (no events, no span slot) until resumed;
 * a host flag, so a timed loop can time the probed launch in some of its steps only */
int niti_model_probe_pause(niti_model_t m, int paused);
/* Weight-gradient probes (phase 2) also time the launch from inside: the kernel min-es its
 * blocks' start and max-es their end on the device wall clock (s_memrealtime); this returns the
 * summed first-block-start -> last-block-end spans and their count, then re-arms. */
int niti_model_probe_read_span(niti_model_t m, double* total_ms, int* count);
/* Runs one layer phase of the last step again on `stream` (phase 0 forward, 1 input gradient,
 * 2 weight gradient; buffers as the step left them, weights untouched), single-device and
 * without the side stream: the isolated measurement next to the in-step probe. */
int niti_model_run_phase(niti_model_t m, int layer, int phase, void* stream);

/* ---- data parallel over RCCL (xGMI) ---------------------------------------------------- */
#define NITI_UNIQUE_ID_BYTES 128
/* rank 0 creates the id; every rank receives it out of band (torch.distributed store). */
int niti_dp_get_unique_id(char id[NITI_UNIQUE_ID_BYTES]);
/* Attach an RCCL communicator (one per model; all its collectives go on the step stream in
 * program order): exact mode all-reduces the input quantiser's statistics (SUM / MAX), every
 * forward and input-gradient range (MAX) and every int32 weight-gradient accumulator (SUM), so
 * N ranks of batch b are bit-identical to one device of batch N*b.  exact=0 keeps the
 * statistics and ranges shard-local (not parity; the gradient SUM stays). */
int niti_model_attach_comm(niti_model_t m, const char id[NITI_UNIQUE_ID_BYTES], int rank, int world, int exact);

/* In-process rank group on ONE device (tests and single-GPU rehearsal of the protocol): each
 * of `world` host threads drives one model attached with its rank; every collective
 * synchronises the caller's stream and the last rank to arrive reduces all ranks' buffers on
 * the device.  Same calls, order and streams as the RCCL path; no second GPU needed. */
typedef struct niti_local_group* niti_local_group_t;
int niti_local_group_create(int world, niti_local_group_t* out);
void niti_local_group_destroy(niti_local_group_t g);
int niti_model_attach_local(niti_model_t m, niti_local_group_t g, int rank, int exact);

/* library build info */
const char* niti_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NITI_HIP_H */
