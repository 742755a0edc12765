"""ctypes binding of libniti_hip.so (the C ABI declared in include/niti_hip.h).

There is no fallback: if the HIP library is missing the import fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# NITI_HIP_LIB selects another build of the same library (diagnostic variants under tools/)
LIB_PATH = os.environ.get("NITI_HIP_LIB") or os.path.join(_HERE, "_lib", "libniti_hip.so")
HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "niti_hip.h")

# MNN::ErrorCode names (include/MNN/ErrorCode.hpp:17-30)
ERROR_NAMES = {0: "NO_ERROR", 1: "OUT_OF_MEMORY", 2: "NOT_SUPPORT", 3: "COMPUTE_SIZE_ERROR",
               4: "NO_EXECUTION", 5: "INVALID_VALUE", 10: "INPUT_DATA_ERROR", 11: "CALL_BACK_STOP"}
NOT_SUPPORT, INVALID_VALUE = 2, 5  # the two codes niti_model_chain_check refuses a layer list with

OP_CONV_INT8 = 700
OP_DECONV_INT8 = 701
OP_RELU_INT8 = 703
OP_RELUGRAD_INT8 = 704
OP_MAXPOOL_INT8 = 705
OP_POOLGRAD_INT8 = 706
OP_LOSS_INT8 = 710
OP_LOSS_GRAD_INT8 = 711
OP_MATMUL_INT8 = 713
OP_PAD_INT8 = 714
OP_LEFTPOOLGRAD_INT8 = 718
OP_GRADIENT_CONV_INT8 = 715
OP_DSP_CONV_INT8 = 800
OP_DSP_RELU_INT8 = 801
OP_DSP_MAXPOOL_INT8 = 802
OP_DSP_RESHAPE_INT8 = 803
OP_DSP_LOSSGRAD_INT8 = 804
OP_DSP_RELUGRAD_INT8 = 805
OP_DSP_MAXPOOLGRAD_INT8 = 807
OP_DSP_TRANSPOSE_INT8 = 808
OP_DSP_WEIGHTROTATE180_INT8 = 809
OP_DSP_RESHAPEGRAD_INT8 = 813
OP_DSP_LEFTPOOLGRAD_DECONV_INT8 = 814
OP_DSP_LEFTPOOLGRAD_GRADIENT_INT8 = 815
OP_DSP_NOP_INT8 = 817
OP_DSP_DECONV_INT8 = 811
OP_DSP_MATMUL_GRADIENT_INT8 = 818
OP_DSP_PARALLEL_GRADIENTCONV_INT8 = 820
OP_DSP_GRADIENT_SPLITBATCHCONV_INT8 = 821
OP_DSP_TRANSPOSEGRADIENT_CONV_INT8 = 822
FORMAT_NCHW, FORMAT_NHWC, FORMAT_NC4HW4 = 0, 1, 2
PAD_CAFFE, PAD_VALID, PAD_SAME = 0, 1, 2
ARCH_LENET, ARCH_VGG11, ARCH_VGG16, ARCH_RESNET18 = 1, 2, 3, 4
ARCH_CHAIN = 5  # a model of the caller's own layer list (niti_model_create_chain)
ARCH_RESNET = 6  # a residual network of the caller's own stage list (niti_model_create_resnet)
RESNET_MAX_STAGES, RESNET_MAX_LAYERS = 8, 256  # NITI_RESNET_MAX_STAGES / _LAYERS
CHAIN_MAX_LAYERS = 64  # NITI_CHAIN_MAX_LAYERS (the `4` entry points; 24 through the older ones)


class NitiError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        super().__init__(f"{what}: {ERROR_NAMES.get(code, code)}")


class Tensor(C.Structure):
    _fields_ = [("data", C.c_void_p), ("dims", C.c_int * 4), ("format", C.c_int)]


class ConvCommon(C.Structure):
    _fields_ = [("kernel_x", C.c_int), ("kernel_y", C.c_int), ("stride_x", C.c_int), ("stride_y", C.c_int),
                ("dilate_x", C.c_int), ("dilate_y", C.c_int), ("pad_x", C.c_int), ("pad_y", C.c_int),
                ("has_pads", C.c_int), ("pads", C.c_int * 4), ("pad_mode", C.c_int),
                ("input_count", C.c_int), ("output_count", C.c_int), ("group", C.c_int)]


class Geom(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "n", "c_in", "h", "w", "c_out", "kh", "kw", "stride_h", "stride_w", "pad_t", "pad_l", "pad_b",
        "pad_r", "dilate_h", "dilate_w", "oh", "ow", "cip", "cop", "np")]


class WgradP16Job(C.Structure):
    """niti_wgrad_p16_job: one weight gradient of niti_conv_wgrad_p16_many."""
    _fields_ = [("g", Geom), ("x_p16", C.c_void_p), ("dy_p16", C.c_void_p), ("acc", C.c_void_p),
                ("amax", C.c_void_p)]


class SgdCombineJob(C.Structure):
    """niti_sgd_combine_job: one split-K slab sum of niti_sgd_combine."""
    _fields_ = [("slab", C.c_void_p), ("splits", C.c_int), ("stride", C.c_int64), ("n", C.c_int64),
                ("acc", C.c_void_p), ("amax", C.c_void_p)]


class SgdJob(C.Structure):
    """niti_sgd_job: one layer's update of niti_sgd_update_many."""
    _fields_ = ([("acc", C.c_void_p), ("amax", C.c_void_p)] +
                [(n, C.c_int) for n in ("rule", "co", "ci", "kk", "cip", "cop")] +
                [(n, C.c_void_p) for n in ("w_ohwi16", "wt_ihwo16", "g_out", "wf", "wft")])


class SgdBitsJob(C.Structure):
    """niti_sgd_bits_job: one layer's update of niti_sgd_update_many_bits."""
    _fields_ = ([("job", SgdJob), ("subw", C.c_void_p)] +
                [(n, C.c_int) for n in ("sub_kh", "sub_kw", "sub_pt", "sub_pl")] +
                [("slab", C.c_void_p), ("splits", C.c_int), ("slab_stride", C.c_int64)])


class Conv0Out(C.Structure):
    """niti_conv0_out: the outputs and options of niti_conv0_fwd."""
    _fields_ = ([(n, C.c_void_p) for n in ("out", "pool_out", "pool_code", "pool_c32", "out_c32", "exp_in",
                                           "wscale", "exp_out")] + [("relu", C.c_int)])


class ChainLayer(C.Structure):
    """niti_chain_layer: one layer of a user-defined chain network."""
    _fields_ = [(n, C.c_int) for n in ("c_out", "kernel", "stride", "pad", "relu", "pool", "flatten")]


class ChainLayer2(C.Structure):
    """niti_chain_layer2: niti_chain_layer's fields and `depthwise`."""
    _fields_ = [(n, C.c_int) for n in ("c_out", "kernel", "stride", "pad", "relu", "pool", "flatten", "depthwise")]


class ChainLayer3(C.Structure):
    """niti_chain_layer3: niti_chain_layer2's fields, `skip` and `gpool`."""
    _fields_ = [(n, C.c_int) for n in ("c_out", "kernel", "stride", "pad", "relu", "pool", "flatten", "depthwise",
                                       "skip", "gpool")]


class DwconvOut(C.Structure):
    """niti_dwconv_out: the outputs and options of niti_dwconv_fwd / niti_dwconv_dgrad."""
    _fields_ = [(n, C.c_void_p) for n in ("out", "relu_mask", "exp_in", "wscale", "exp_out")] + [("relu", C.c_int)]


class ResnetSpec(C.Structure):
    """niti_resnet_spec: the stage list of a user-defined residual network."""
    _fields_ = ([(n, C.c_int) for n in ("in_c", "stem_kernel", "stem_stride", "stem_pad", "stem_pool", "width",
                                        "n_stages")] +
                [("depths", C.c_int * RESNET_MAX_STAGES), ("classes", C.c_int)])


class EvalTotals(C.Structure):
    """niti_eval_totals: the running totals of an evaluation pass."""
    _fields_ = [("images", C.c_uint64), ("top1", C.c_uint64), ("topk", C.c_uint64), ("loss_sum", C.c_double)]


class RequantFused(C.Structure):
    """niti_requant_fused: the options of niti_requant_act_fused."""
    _fields_ = ([(n, C.c_void_p) for n in (
        "exp_in", "wscale", "exp_out", "relu_mask", "out_nhwc16", "pool_out", "pool_x", "pool_y", "pool_dx",
        "pool_dx_c32", "out_p16", "pool3_out", "pool3_arg")] + [(n, C.c_int) for n in (
            "relu", "pool_relu", "pool_h", "pool_w", "zero_cls", "zc_h", "zc_w", "pool3_h", "pool3_w", "pool3_oh",
            "pool3_ow")])


_lib = None


def header_functions():
    """Every function the public header declares (name -> None)."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\*?\s+\*?(niti_[a-z0-9_]+)\s*\(", src, flags=re.M)))


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libniti_hip.so not built ({LIB_PATH}); run __graft_entry__.build() or "
                          f"make -C mandheling-dsp-training_amd/csrc")
    # torch ships its own libamdhip64.so.7 (same soname as /opt/rocm's).  Load torch first so
    # this library binds to the runtime torch uses; loaded the other way round, torch is bound to
    # /opt/rocm's copy and the first allocation in the process fails (seen on the GPU box).
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, ci = C.c_void_p, C.c_int32, C.c_int64, C.c_int
    tp = C.POINTER(Tensor)
    sig = {
        "niti_version": (C.c_char_p, []),
        "niti_create_execution": (ci, [ci, C.POINTER(ConvCommon), C.POINTER(vp)]),
        "niti_execution_resize": (ci, [vp, tp, ci, tp, ci]),
        "niti_execution_execute": (ci, [vp, tp, ci, tp, ci, vp]),
        "niti_destroy_execution": (None, [vp]),
        "niti_execution_workspace_bytes": (C.c_size_t, [vp]),
        "niti_execution_status": (ci, [vp, vp]),
        "niti_diag_rowconv_barrier": (None, [C.c_uint32, C.c_uint32]),
        "niti_diag_rowconv_speculate": (None, [C.c_int]),
        "niti_diag_rowconv_rows1": (None, [C.c_int]),
        "niti_diag_gemm_speculate": (None, [C.c_int]),
        "niti_diag_gemm_fused_launches": (C.c_ulonglong, []),
        "niti_diag_head_chain_launches": (C.c_ulonglong, []),
        "niti_diag_head_chain": (None, [C.c_int]),
        "niti_diag_p16_jobs_cap": (None, [C.c_int]),
        "niti_diag_wgrad_batch": (None, [C.c_int]),
        "niti_diag_wgrad_batch_launches": (C.c_ulonglong, []),
        "niti_diag_wgrad_quad": (None, [C.c_int]),
        "niti_conv_wgrad_p16_many_items": (ci, [C.POINTER(WgradP16Job), ci, ci, ci, C.POINTER(ci), ci, C.POINTER(ci),
                                                ci, C.POINTER(ci)]),
        "niti_tensor_convert": (ci, [tp, tp, vp]),
        "niti_geom_finalize": (ci, [C.POINTER(Geom)]),
        "niti_conv_workspace_bytes": (ci, [C.POINTER(Geom), ci, C.POINTER(C.c_size_t)]),
        "niti_matmul_workspace_bytes": (ci, [ci, ci, ci, C.POINTER(C.c_size_t)]),
        "niti_conv_plan_info": (ci, [C.POINTER(Geom), ci, C.c_size_t, C.POINTER(C.c_int)]),
        "niti_conv_fwd_acc": (ci, [C.POINTER(Geom), vp, vp, vp, vp, vp, C.c_size_t, vp]),
        "niti_conv_dgrad_acc": (ci, [C.POINTER(Geom), vp, vp, vp, vp, vp, C.c_size_t, vp]),
        "niti_conv_wgrad_acc": (ci, [C.POINTER(Geom), vp, vp, vp, vp, vp, C.c_size_t, vp]),
        "niti_conv_fwd_phase1": (ci, [C.POINTER(Geom), vp, vp, vp, vp, vp, C.c_size_t, vp]),
        "niti_conv_rows_ok": (ci, [C.POINTER(Geom)]),
        "niti_conv_rows_plan": (ci, [C.POINTER(Geom), ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]),
        "niti_conv_rows_plan2": (ci, [C.POINTER(Geom), ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci),
                                      C.POINTER(ci)]),
        "niti_nhwc16_to_c32": (ci, [vp, ci, ci, ci, ci, vp, vp]),
        "niti_weights_to_wf": (ci, [vp, ci, ci, ci, ci, vp, vp]),
        "niti_conv_fwd_rows": (ci, [C.POINTER(Geom), vp, vp, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, C.c_uint32, vp,
                                    vp]),
        "niti_conv_dgrad_rows": (ci, [C.POINTER(Geom), vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, C.c_uint32, vp, vp]),
        "niti_rows_spec_slot": (vp, [vp, ci]),
        "niti_conv_fwd_phase2": (ci, [C.POINTER(Geom), vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, C.c_size_t, vp]),
        "niti_conv_dgrad_phase1": (ci, [C.POINTER(Geom), vp, vp, vp, vp, vp, C.c_size_t, vp]),
        "niti_conv_dgrad_phase2": (ci, [C.POINTER(Geom), vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, C.c_size_t, vp]),
        "niti_nhwc16_to_p16": (ci, [vp, i64, ci, vp, vp]),
        "niti_diag_wgrad_stamps": (None, [vp]),
        "niti_diag_rowconv_stamps": (None, [vp]),
        "niti_conv_wgrad_p16_workspace": (ci, [C.POINTER(Geom), ci, C.POINTER(C.c_size_t)]),
        "niti_conv_wgrad_p16_acc": (ci, [C.POINTER(Geom), vp, vp, vp, vp, vp, C.c_size_t, ci, vp]),
        "niti_conv_wgrad_p16_many_workspace": (ci, [C.POINTER(WgradP16Job), ci, ci, ci, C.POINTER(C.c_size_t)]),
        "niti_conv_wgrad_p16_many": (ci, [C.POINTER(WgradP16Job), ci, ci, ci, vp, C.c_size_t, C.POINTER(ci), vp]),
        "niti_matmul_acc": (ci, [ci, ci, ci, vp, i64, vp, i64, vp, i64, vp, vp, C.c_size_t, vp]),
        "niti_absmax_i32": (ci, [vp, i64, vp, vp]),
        "niti_requant_act": (ci, [vp, i64, ci, vp, vp, vp, vp, ci, vp, vp, vp]),
        "niti_requant_act_fused": (ci, [vp, i64, ci, vp, C.POINTER(RequantFused), vp]),
        "niti_requant_grad": (ci, [vp, i64, vp, ci, vp, vp, vp]),
        "niti_sgd_update": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp]),
        "niti_sgd_combine": (ci, [C.POINTER(SgdCombineJob), ci, vp]),
        "niti_sgd_update_many": (ci, [C.POINTER(SgdJob), ci, vp]),
        "niti_sgd_update_many_bits": (ci, [C.POINTER(SgdBitsJob), ci, vp, vp]),
        "niti_model_set_update_bits": (ci, [vp, ci, ci, vp]),
        "niti_model_get_update_bits": (ci, [vp, C.POINTER(i32), vp]),
        "niti_input_im2col": (ci, [vp] + [ci] * 9 + [vp, i64, vp, vp, vp, vp, ci, ci, vp, vp]),
        "niti_conv0_fwd": (ci, [C.POINTER(Geom), vp, vp, vp, C.POINTER(Conv0Out), ci, vp]),
        "niti_diag_conv0_blocks": (None, [C.c_int]),
        "niti_conv0_wgrad_codes": (ci, [ci, ci, ci, ci, ci, vp, vp, vp, ci, vp, C.c_size_t, C.POINTER(ci), vp]),
        "niti_conv0_wgrad_codes_slabs": (ci, [ci, ci, ci, ci, ci, ci]),
        "niti_diag_conv0_wgrad_blocks": (None, [C.c_int]),
        "niti_diag_conv0_wgrad_codes": (None, [C.c_int]),
        "niti_diag_conv0_wgrad_codes_launches": (C.c_ulonglong, []),
        "niti_dwconv_ok": (ci, [C.POINTER(Geom)]),
        "niti_dwconv_fwd": (ci, [C.POINTER(Geom), vp, vp, vp, C.POINTER(DwconvOut), ci, vp]),
        "niti_dwconv_dgrad": (ci, [C.POINTER(Geom), vp, vp, vp, C.POINTER(DwconvOut), ci, vp]),
        "niti_dwconv_wgrad": (ci, [C.POINTER(Geom), vp, vp, vp, C.c_size_t, C.POINTER(ci), vp]),
        "niti_dwconv_wgrad_slabs": (ci, [C.POINTER(Geom)]),
        "niti_dwconv_wgrad_reduce": (ci, [C.POINTER(Geom), vp, ci, vp, vp, vp]),
        "niti_dwconv2_ok": (ci, [C.POINTER(Geom)]),
        "niti_dwconv2_fwd": (ci, [C.POINTER(Geom), vp, vp, vp, C.POINTER(DwconvOut), ci, vp]),
        "niti_dwconv2_dgrad": (ci, [C.POINTER(Geom), vp, vp, vp, C.POINTER(DwconvOut), ci, vp]),
        "niti_dwconv2_wgrad": (ci, [C.POINTER(Geom), vp, vp, vp, C.c_size_t, C.POINTER(ci), vp]),
        "niti_dwconv2_wgrad_slabs": (ci, [C.POINTER(Geom)]),
        "niti_dwconv2_wgrad_reduce": (ci, [C.POINTER(Geom), vp, ci, vp, vp, vp]),
        "niti_nhwc16_to_chwn16": (ci, [vp, ci, ci, ci, ci, vp, vp]),
        "niti_ohwi16_to_ihwo16": (ci, [vp, ci, ci, ci, ci, ci, vp, vp]),
        "niti_nchw_to_nhwc16": (ci, [vp, ci, ci, ci, ci, vp, vp]),
        "niti_nchw_to_chwn16": (ci, [vp, ci, ci, ci, ci, ci, vp, vp]),
        "niti_nhwc16_to_nchw": (ci, [vp, ci, ci, ci, ci, vp, vp]),
        "niti_oihw_to_ohwi16": (ci, [vp, ci, ci, ci, ci, vp, vp]),
        "niti_ohwi16_to_oihw": (ci, [vp, ci, ci, ci, ci, vp, vp]),
        "niti_residual_add": (ci, [vp, vp, vp, vp, i64, vp, vp, vp, vp]),
        "niti_residual_requant": (ci, [vp, vp, vp, vp, i64, vp, vp, vp, ci, vp, vp]),
        "niti_residual_requant_relu_grad": (ci, [vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]),
        "niti_sum_pool": (ci, [vp, ci, ci, ci, vp, vp, vp]),
        "niti_sum_pool_wide": (ci, [vp, ci, ci, ci, vp, vp, vp]),
        "niti_sum_pool_grad": (ci, [vp, ci, ci, ci, vp, vp]),
        "niti_im2col": (ci, [C.POINTER(Geom), vp, ci, vp, vp]),
        "niti_im2col_nchw": (ci, [C.POINTER(Geom), vp, ci, vp, vp]),
        "niti_sgd_update_wf": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]),
        "niti_conv_rows_nhwc_ok": (ci, [C.POINTER(Geom), ci]),
        "niti_conv_plan_set": (ci, [C.POINTER(Geom), ci, vp]),
        "niti_maxpool": (ci, [vp] + [ci] * 7 + [vp, ci, ci, vp]),
        "niti_maxpool_grad": (ci, [vp, vp, vp] + [ci] * 10 + [vp, vp]),
        "niti_maxpool_grad_ws": (ci, [vp, vp, vp] + [ci] * 10 + [vp, vp, vp]),
        "niti_maxpool_arg": (ci, [vp] + [ci] * 7 + [vp, ci, ci, vp, vp]),
        "niti_maxpool_grad_arg": (ci, [vp, vp, vp] + [ci] * 10 + [vp, vp, vp]),
        "niti_relu_grad": (ci, [vp, vp, i64, vp, vp]),
        "niti_loss_grad": (ci, [vp, ci, ci, ci, vp, vp, vp, vp]),
        "niti_head_metrics": (ci, [vp, ci, ci, ci, vp, vp, ci, vp, vp, vp, vp, C.c_size_t, vp]),
        "niti_head_metrics_workspace": (ci, [ci, C.POINTER(C.c_size_t)]),
        "niti_model_eval_step": (ci, [vp, vp, ci, vp, vp]),
        "niti_model_eval_step_images": (ci, [vp, vp, vp, vp]),
        "niti_model_eval_reset": (ci, [vp, vp]),
        "niti_model_eval_read": (ci, [vp, C.POINTER(EvalTotals), vp]),
        "niti_model_eval_topk": (ci, [vp, ci]),
        "niti_model_get_predictions": (ci, [vp, vp, vp]),
        "niti_model_copy_weights": (ci, [vp, vp, vp]),
        "niti_model_create": (ci, [ci, ci, C.POINTER(vp)]),
        "niti_model_create2": (ci, [ci, ci, ci, C.POINTER(vp)]),
        "niti_model_create3": (ci, [ci, ci, ci, ci, C.POINTER(vp)]),
        # (layers: a ChainLayer array, passed untyped)
        "niti_model_chain_check": (ci, [vp, ci, ci, ci, vp]),
        "niti_model_create_chain": (ci, [vp, ci, ci, ci, ci, C.POINTER(vp)]),
        # (layers: a ChainLayer2 array, passed untyped)
        "niti_model_chain_check2": (ci, [vp, ci, ci, ci, vp]),
        "niti_model_create_chain2": (ci, [vp, ci, ci, ci, ci, C.POINTER(vp)]),
        "niti_model_layer_depthwise": (ci, [vp, ci]),
        "niti_model_chain_check3": (ci, [vp, ci, ci, ci, vp]),
        "niti_model_create_chain3": (ci, [vp, ci, ci, ci, ci, C.POINTER(vp)]),
        "niti_model_chain_check4": (ci, [vp, ci, ci, ci, vp]),
        "niti_model_create_chain4": (ci, [vp, ci, ci, ci, ci, C.POINTER(vp)]),
        "niti_model_layer_skip": (ci, [vp, ci, C.POINTER(ci), C.POINTER(ci)]),
        # (spec: a ResnetSpec, passed untyped)
        "niti_model_resnet_check": (ci, [vp, ci, C.POINTER(ci), vp]),
        "niti_model_create_resnet": (ci, [vp, ci, ci, C.POINTER(vp)]),
        "niti_model_destroy": (None, [vp]),
        "niti_model_num_layers": (ci, [vp]),
        "niti_model_layer_info": (ci, [vp, ci, C.POINTER(ci)]),
        "niti_model_set_weight": (ci, [vp, ci, vp, ci]),
        "niti_model_get_weight": (ci, [vp, ci, vp]),
        "niti_model_train_step": (ci, [vp, vp, ci, vp, vp]),
        "niti_model_get_logits": (ci, [vp, vp, C.POINTER(ci), vp]),
        "niti_model_get_tap": (ci, [vp, ci, ci, vp, C.c_size_t, vp]),
        "niti_model_step_macs": (i64, [vp]),
        "niti_model_set_graph": (ci, [vp, ci]),
        "niti_model_set_rowconv": (ci, [vp, ci]),
        "niti_model_keep_grads": (ci, [vp, ci]),
        "niti_model_rowconv_error": (ci, [vp]),
        "niti_model_spec_stats": (ci, [vp, vp, ci]),
        "niti_model_autotune": (ci, [vp, ci, vp]),
        "niti_model_set_overlap": (ci, [vp, ci]),
        "niti_model_plan_info": (ci, [vp, ci, ci, C.POINTER(ci)]),
        "niti_model_plan_set": (ci, [vp, ci, ci, C.POINTER(ci)]),
        "niti_plan_reset": (None, []),
        "niti_model_set_probe": (ci, [vp, ci, ci, ci]),
        "niti_model_probe_read": (ci, [vp, C.POINTER(C.c_double), C.POINTER(ci)]),
        "niti_model_probe_pause": (ci, [vp, ci]),
        "niti_model_spec_slot": (ci, [vp, ci, ci, C.POINTER(C.c_uint32)]),
        "niti_model_run_phase": (ci, [vp, ci, ci, vp]),
        "niti_model_probe_read_span": (ci, [vp, C.POINTER(C.c_double), C.POINTER(ci)]),
        "niti_dp_get_unique_id": (ci, [C.c_char_p]),
        "niti_model_attach_comm": (ci, [vp, C.c_char_p, ci, ci, ci]),
        "niti_image_stats": (ci, [vp, i64, vp, vp]),
        "niti_image_quantize": (ci, [vp, ci, ci, ci, vp, i64, vp, vp, vp]),
        "niti_image_quantize_nhwc16": (ci, [vp, ci, ci, ci, ci, vp, i64, vp, vp, vp]),
        "niti_model_train_step_images": (ci, [vp, vp, vp, vp]),
        "niti_model_get_input": (ci, [vp, vp, C.POINTER(ci), vp]),
        "niti_dataset_create": (ci, [vp, vp, i64, ci, ci, ci, C.POINTER(vp)]),
        "niti_dataset_destroy": (None, [vp]),
        "niti_dataset_order_check": (ci, [vp, vp, i64, i64, ci, ci]),
        "niti_dataset_set_order": (ci, [vp, vp, vp, i64]),
        "niti_dataset_set_output": (ci, [vp, ci, ci]),
        "niti_dataset_windows_check": (ci, [vp, vp, i64, ci, ci]),
        "niti_dataset_set_order_windows": (ci, [vp, vp, vp, vp, i64]),
        "niti_batch_gather": (ci, [vp, i64, ci, vp, vp, vp]),
        "niti_model_train_steps_dataset": (ci, [vp, vp, i64, ci, vp]),
        "niti_model_eval_steps_dataset": (ci, [vp, vp, i64, ci, vp]),
        "niti_model_train_metrics": (ci, [vp, ci]),
        "niti_model_train_metrics_reset": (ci, [vp, vp]),
        "niti_model_train_metrics_read": (ci, [vp, C.POINTER(EvalTotals), vp]),
        "niti_local_group_create": (ci, [ci, C.POINTER(vp)]),
        "niti_local_group_destroy": (None, [vp]),
        "niti_model_attach_local": (ci, [vp, vp, ci, ci]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def check(code, what=""):
    if code != 0:
        raise NitiError(code, what)
