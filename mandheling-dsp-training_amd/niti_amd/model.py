"""Device-resident NITI training step (section 3 of include/niti_hip.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._lib import check
from .ops import _stream


class NitiModel:
    """NITIInt8Train's model + NITI_SGD step, on one GPU (optionally one rank of a DP group)."""

    def __init__(self, arch: int, batch: int, in_hw: int = 0, classes: int = 0):
        """arch: niti_amd.ARCH_*; in_hw: the input size (0: the architecture's); classes: the head's
        class count (0: the architecture's; ResNet-18 only)."""
        self._lib = L.lib()
        h = C.c_void_p()
        check(self._lib.niti_model_create3(arch, batch, int(in_hw), int(classes), C.byref(h)), "model_create")
        self._adopt(h, arch, batch)

    def _adopt(self, h, arch: int, batch: int):
        """The Python side of a ready handle (niti_model_create3's or niti_model_create_chain's)."""
        self._h = h
        self.arch, self.batch = arch, batch
        self.chain = None  # from_chain: the normalised layer list
        self.resnet = None  # from_resnet: the normalised stage list
        self._wscale = {}
        self.layers = []
        for i in range(self._lib.niti_model_num_layers(h)):
            info = (C.c_int * 12)()
            check(self._lib.niti_model_layer_info(h, i, info), "layer_info")
            keys = ("c_in", "c_out", "kh", "kw", "h", "w", "oh", "ow", "pad", "stride", "relu", "pool")
            self.layers.append(dict(zip(keys, list(info))))
            self.layers[-1]["depthwise"] = 1 if self._lib.niti_model_layer_depthwise(h, i) == 1 else 0

    @classmethod
    def from_chain(cls, spec, in_c: int, in_hw: int, batch: int) -> "NitiModel":
        """A model of the caller's own chain network (niti_model_create_chain2; _create_chain3 for a list
        with a strided layer, _create_chain4 for one with a skip, a global pool or more than 24 layers): spec is a
        list of dicts (c_out, kernel[, pad, relu, pool, flatten, depthwise, stride, skip, gpool]) or tuples in
        that order, over in_c x in_hw x in_hw inputs; the last layer's c_out is the
        class count.  A depthwise layer (3x3 or 5x5, c_out 0 or its input's channels) has weights
        [C, 1, k, k]; stride (1 or 2) is a dense or depthwise layer's own; skip = d adds the final output of
        the layer d places back to the layer's conv output, ahead of its relu; gpool = 1 sums the layer's map
        into a 1x1 map; such a list may have up to 64 layers.  ValueError for a
        malformed list, NitiError (NOT_SUPPORT) for one the library does not run -- nothing is
        allocated then.  The model reports arch ARCH_CHAIN; .chain holds the normalised spec."""
        from .chain import entry_points, normalize_spec, to_c
        spec = normalize_spec(spec)
        arr, n = to_c(spec)
        m = cls.__new__(cls)
        m._lib = L.lib()
        h = C.c_void_p()
        create = entry_points(spec)[1]
        code = create(arr, n, int(in_c), int(in_hw), int(batch), C.byref(h))
        if code == L.INVALID_VALUE:
            raise ValueError(f"malformed layer list for a {in_c} x {in_hw} x {in_hw} input at batch {batch}: {spec}")
        check(code, "model_create_chain")
        m._adopt(h, L.ARCH_CHAIN, batch)
        for i, (d, l) in enumerate(zip(spec, m.layers)):  # (a depthwise layer's c_out as derived, whatever normalize_spec could tell)
            d["c_out"] = l["c_out"]
            if "skip" in d or "gpool" in d:  # (reported for the lists that use them: niti_model_layer_skip)
                sk, gp = C.c_int(), C.c_int()
                check(m._lib.niti_model_layer_skip(h, i, C.byref(sk), C.byref(gp)), "layer_skip")
                for k, v in (("skip", sk.value), ("gpool", gp.value)):
                    if k in d:
                        l[k] = v
        m.chain, m.in_c, m.in_hw = spec, int(in_c), int(in_hw)
        return m

    @classmethod
    def from_resnet(cls, spec, in_hw: int, batch: int, **kw) -> "NitiModel":
        """A residual network of the caller's own stage list (niti_model_create_resnet): spec is a
        dict as niti_amd.normalize_resnet_spec takes (keywords override its entries), over
        in_c x in_hw x in_hw inputs.
        ValueError for a malformed spec, NitiError (NOT_SUPPORT) for one the library does not run --
        nothing is allocated then.  The model reports arch ARCH_RESNET; .resnet holds the normalised
        spec."""
        from .resnet import normalize_resnet_spec, to_c
        spec = normalize_resnet_spec(spec, **kw)
        cs = to_c(spec)
        m = cls.__new__(cls)
        m._lib = L.lib()
        h = C.c_void_p()
        code = m._lib.niti_model_create_resnet(C.byref(cs), int(in_hw), int(batch), C.byref(h))
        if code == L.INVALID_VALUE:
            raise ValueError(f"malformed residual network for a {in_hw} x {in_hw} input at batch {batch}: {spec}")
        check(code, "model_create_resnet")
        m._adopt(h, L.ARCH_RESNET, batch)
        m.resnet, m.in_hw = spec, int(in_hw)
        return m

    def _resnet_record(self):
        from .checkpoint import resnet_record
        return None if self.resnet is None else resnet_record(self.resnet, self.in_hw)

    def _chain_record(self):
        from .checkpoint import chain_record
        return None if self.chain is None else chain_record(self.chain, self.in_c, self.in_hw)

    def init_weights(self, seed: int):
        """Every layer's weights and scale from the reference's initialiser (niti_amd.init.xavier_int8),
        one default_rng(seed) consumed in layer order."""
        from .init import xavier_int8
        rng = np.random.default_rng(seed)
        for i in range(len(self.layers)):
            w, s = xavier_int8(self.weight_shape(i), rng)
            self.set_weight(i, w, s)

    def weight_shape(self, i):
        l = self.layers[i]
        if l["depthwise"]:  # (NN.cpp:1118-1125: {C, 1, kh, kw} with group = C)
            return (l["c_out"], 1, l["kh"], l["kw"])
        return (l["c_out"], l["c_in"], l["kh"], l["kw"])

    def set_weight(self, i, w: np.ndarray, wscale: int):
        if not 0 <= i < len(self.layers):
            raise ValueError(f"layer {i} out of range (model has {len(self.layers)})")
        w = np.asarray(w)
        if w.dtype != np.int8 or tuple(w.shape) != self.weight_shape(i):
            # checked here, not by an assert: the C ABI copies weight_shape(i) bytes from w
            raise ValueError(f"layer {i}: weight {w.dtype} {tuple(w.shape)}, want int8 {self.weight_shape(i)}")
        w = np.ascontiguousarray(w)
        check(self._lib.niti_model_set_weight(self._h, i, w.ctypes.data_as(C.c_void_p), int(wscale)), "set_weight")
        self._wscale[i] = int(wscale)

    def save(self, path: str):
        """Snapshot the device weights + wscales (mnistTrain.cpp:375-376 `Variable::save`)."""
        from .checkpoint import save_params
        if len(self._wscale) != len(self.layers):
            raise ValueError("save() before every layer's weight was set")
        save_params(path, [self.get_weight(i) for i in range(len(self.layers))],
                    [self._wscale[i] for i in range(len(self.layers))], self.arch,
                    in_hw=self.layers[0]["h"], chain=self._chain_record(), resnet=self._resnet_record(),
                    update_bits=self.update_bits())

    def load(self, path: str):
        """Restore a snapshot written by save() into this model's device weights."""
        from .checkpoint import check_update_bits, expect_chain, load_chain, load_params, load_update_bits
        weights, wscales, arch = load_params(path)
        if arch != self.arch or len(weights) != len(self.layers):
            raise ValueError(f"snapshot is arch {arch} with {len(weights)} layers, model is arch {self.arch}")
        if self.chain is not None:
            expect_chain(load_chain(path), self._chain_record(), path)
        if self.resnet is not None:
            from .checkpoint import load_resnet
            expect_chain(load_resnet(path), self._resnet_record(), path)
        # every layer's shape before any device write (a VGG-16 snapshot taken at another input
        # size has the same arch and layer count but a different first FC layer)
        for i, w in enumerate(weights):
            if tuple(w.shape) != self.weight_shape(i):
                raise ValueError(f"snapshot layer {i} is {tuple(w.shape)}, model layer is {self.weight_shape(i)}")
        bits = check_update_bits(load_update_bits(path), len(self.layers), path)
        for i, (w, s) in enumerate(zip(weights, wscales)):
            self.set_weight(i, w, s)
        if bits is not None:  # (a snapshot without the key leaves the model's own)
            self.set_update_bits(bits)

    def save_mnn(self, path: str):
        """The reference's own snapshot: `Variable::save(model->parameters(), path)` -- an MNN Net
        flatbuffer of one TrainableParam Blob per layer weight (int8 OIHW, express/Expr.cpp:833-965)
        -- plus `path.wscale.json` with the weight scales the NITI modules keep outside their
        parameters.  `Variable::load` + `Module::loadParameters` read the .mnn unchanged."""
        from . import mnn_snapshot
        if len(self._wscale) != len(self.layers):
            raise ValueError("save_mnn() before every layer's weight was set")
        mnn_snapshot.save(path, [self.get_weight(i) for i in range(len(self.layers))],
                          [self._wscale[i] for i in range(len(self.layers))],
                          meta=self._mnn_meta())

    def _mnn_meta(self):
        meta = {"arch": int(self.arch), "in_hw": int(self.layers[0]["h"])}
        if self.chain is not None:
            meta["chain"] = self._chain_record()
        if self.resnet is not None:
            meta["resnet"] = self._resnet_record()
        bits = self.update_bits()
        if any(b != 2 for b in bits):  # (a default model's side-car stays what it always was)
            meta["update_bits"] = bits
        return meta

    def load_mnn(self, path: str):
        """`Module::loadParameters(Variable::load(path))` (mnistTrain.cpp:375-376): the weights in
        file order; the wscales from the side-car when there is one, otherwise the model keeps its
        own (as the reference's modules do).  Every shape is checked before any device write."""
        from . import mnn_snapshot
        weights, wscales, meta = mnn_snapshot.load(path)
        if self.chain is not None:
            from .checkpoint import expect_chain
            expect_chain(mnn_snapshot.chain_of(meta), self._chain_record(), path)
        if self.resnet is not None:
            from .checkpoint import expect_chain
            expect_chain(mnn_snapshot.resnet_of(meta), self._resnet_record(), path)
        if len(weights) != len(self.layers):
            raise ValueError(f"{path}: {len(weights)} parameters, model has {len(self.layers)} layers")
        for i, w in enumerate(weights):
            if tuple(w.shape) != self.weight_shape(i):
                raise ValueError(f"snapshot parameter {i} is {tuple(w.shape)}, model layer is {self.weight_shape(i)}")
        if wscales is None:
            if len(self._wscale) != len(self.layers):
                raise ValueError(f"{path}: no wscale side-car and the model's scales are not set")
            wscales = [self._wscale[i] for i in range(len(self.layers))]
        from .checkpoint import check_update_bits
        bits = check_update_bits((meta or {}).get("update_bits"), len(self.layers), path)
        for i, (w, s) in enumerate(zip(weights, wscales)):
            self.set_weight(i, w, s)
        if bits is not None:
            self.set_update_bits(bits)

    def get_weight(self, i) -> np.ndarray:
        w = np.empty(self.weight_shape(i), np.int8)
        check(self._lib.niti_model_get_weight(self._h, i, w.ctypes.data_as(C.c_void_p)), "get_weight")
        return w

    def train_step(self, x: torch.Tensor, exp_in: int, labels: torch.Tensor, stream=None):
        assert x.dtype == torch.int8 and x.is_contiguous() and labels.dtype == torch.int32
        check(self._lib.niti_model_train_step(self._h, C.c_void_p(x.data_ptr()), int(exp_in),
                                              C.c_void_p(labels.data_ptr()), _stream(stream)), "train_step")

    def train_step_images(self, images: torch.Tensor, labels: torch.Tensor, stream=None):
        """One step from uint8 images [batch][C][H][W]: the input quantiser (MnistUtils.cpp:83-93)
        runs on device and supplies x and its exponent."""
        assert images.dtype == torch.uint8 and images.is_contiguous() and labels.dtype == torch.int32
        check(self._lib.niti_model_train_step_images(self._h, C.c_void_p(images.data_ptr()),
                                                     C.c_void_p(labels.data_ptr()), _stream(stream)),
              "train_step_images")

    def eval_step(self, x: torch.Tensor, exp_in: int, labels: torch.Tensor, stream=None):
        """Forward only (no weight is written): the logits of x on the current weights, their
        argmax / top-k / loss against labels added to the running totals.  labels[i] = -1 excludes
        image i.  Asynchronous."""
        assert x.dtype == torch.int8 and x.is_contiguous() and labels.dtype == torch.int32
        check(self._lib.niti_model_eval_step(self._h, C.c_void_p(x.data_ptr()), int(exp_in),
                                             C.c_void_p(labels.data_ptr()), _stream(stream)), "eval_step")

    def eval_step_images(self, images: torch.Tensor, labels: torch.Tensor, stream=None):
        """eval_step from uint8 images [batch][C][H][W], quantised on device with the batch's own
        statistics (the reference's test loop, MnistUtils.cpp:161-172)."""
        assert images.dtype == torch.uint8 and images.is_contiguous() and labels.dtype == torch.int32
        check(self._lib.niti_model_eval_step_images(self._h, C.c_void_p(images.data_ptr()),
                                                    C.c_void_p(labels.data_ptr()), _stream(stream)),
              "eval_step_images")

    def eval_reset(self, stream=None):
        """Zero the running totals (asynchronous)."""
        check(self._lib.niti_model_eval_reset(self._h, _stream(stream)), "eval_reset")

    def eval_read(self, stream=None) -> dict:
        """The running totals (synchronises): images, top1, topk, loss_sum, and loss = loss_sum /
        images, accuracy = top1 / images (nan before any image was counted)."""
        t = L.EvalTotals()
        check(self._lib.niti_model_eval_read(self._h, C.byref(t), _stream(stream)), "eval_read")
        return self._totals_dict(t)

    @staticmethod
    def _totals_dict(t) -> dict:
        n = int(t.images)
        return {"images": n, "top1": int(t.top1), "topk": int(t.topk), "loss_sum": float(t.loss_sum),
                "loss": float(t.loss_sum) / n if n else float("nan"),
                "accuracy": int(t.top1) / n if n else float("nan")}

    def eval_topk(self, k: int):
        """The k of the totals' topk count for later evaluation steps (default 5, clamped to the
        class count)."""
        check(self._lib.niti_model_eval_topk(self._h, int(k)), "eval_topk")

    def predictions(self, stream=None) -> np.ndarray:
        """int32 [batch]: the first-maximum class of each image of the last evaluation batch."""
        out = np.empty(self.batch, np.int32)
        check(self._lib.niti_model_get_predictions(self._h, out.ctypes.data_as(C.c_void_p), _stream(stream)),
              "get_predictions")
        return out

    # ---- update bits: the learning rate (include/niti_hip.h, "Update bits")
    def set_update_bits(self, bits, stream=None):
        """How many bits of each layer's weight gradient its update keeps -- NITI's learning rate --
        set on the device by a launch on `stream`: in effect for the steps enqueued after it (replays
        of a captured step included).  bits: an int for every layer, a sequence of one value per
        layer, or a dict {layer: bits}; each in 0..7, 2 the default (the reference's rule), 0 a
        frozen layer.  Everything is checked before the first launch.  Data parallel: set the same
        values on every rank (a mismatch is not detected)."""
        n = len(self.layers)
        if isinstance(bits, dict):
            items = [(int(k), v) for k, v in bits.items()]
        elif isinstance(bits, (int, np.integer)):
            items = [(-1, bits)]
        else:
            bits = list(bits)
            if len(bits) != n:
                raise ValueError(f"{len(bits)} update bits for a model of {n} layers")
            items = list(enumerate(bits))
        for layer, b in items:
            if not isinstance(b, (int, np.integer)) or isinstance(b, bool) or not 0 <= int(b) <= 7:
                raise ValueError(f"update bits {b!r}: an int in 0..7")
            if not -1 <= layer < n or (layer == -1 and len(items) != 1):
                raise ValueError(f"layer {layer} out of range (model has {n})")
        for layer, b in items:
            check(self._lib.niti_model_set_update_bits(self._h, layer, int(b), _stream(stream)), "set_update_bits")

    def update_bits(self, stream=None) -> list:
        """Every layer's update bits, read back from the device (synchronises)."""
        out = (C.c_int32 * len(self.layers))()
        check(self._lib.niti_model_get_update_bits(self._h, out, _stream(stream)), "get_update_bits")
        return [int(v) for v in out]

    def copy_weights_from(self, other: "NitiModel", stream=None):
        """Device-to-device copy of every layer's weights and weight scale from a model of the same
        architecture, input size and class count (the batch may differ).  The update bits are not
        copied (the copy's use is an evaluation model)."""
        check(self._lib.niti_model_copy_weights(self._h, other._h, _stream(stream)), "copy_weights")
        self._wscale = dict(other._wscale)

    def evaluate(self, images, labels, stream=None) -> dict:
        """Evaluate a whole set of uint8 images [N][C][H][W] with int labels [N] (numpy arrays or
        tensors): resets the totals, runs eval_step_images batch by batch -- the last partial batch
        padded with zero images and label -1 -- and synchronises once, in eval_read."""
        img = torch.as_tensor(images)
        lab = torch.as_tensor(labels).to(torch.int32)
        assert img.dtype == torch.uint8 and img.shape[0] == lab.shape[0]
        n, b = int(img.shape[0]), self.batch
        pad = (-n) % b
        if pad:
            img = torch.cat([img, torch.zeros((pad,) + tuple(img.shape[1:]), dtype=torch.uint8, device=img.device)])
            lab = torch.cat([lab, torch.full((pad,), -1, dtype=torch.int32, device=lab.device)])
        img = img.cuda().contiguous()
        lab = lab.cuda().contiguous()
        self.eval_reset(stream)
        for i in range(0, n + pad, b):
            self.eval_step_images(img[i:i + b], lab[i:i + b], stream)
        return self.eval_read(stream)

    # ---- device-resident dataset (niti_amd.dataset)
    def train_steps(self, ds, first_step: int, n_steps: int, stream=None):
        """n_steps training steps on batches first_step.. of ds's order, gathered on the device
        (niti_model_train_steps_dataset).  Asynchronous: nothing waits on the host."""
        check(self._lib.niti_model_train_steps_dataset(self._h, ds._h, int(first_step), int(n_steps), _stream(stream)),
              "train_steps_dataset")

    def eval_steps(self, ds, first_step: int, n_steps: int, stream=None):
        """The same through the evaluation step; entries of index -1 are counted nowhere."""
        check(self._lib.niti_model_eval_steps_dataset(self._h, ds._h, int(first_step), int(n_steps), _stream(stream)),
              "eval_steps_dataset")

    def fit_epoch(self, ds, seed: int, epoch: int, pad: int = 0, flip: bool = False, stream=None, rrc=None,
                  update_bits=None) -> int:
        """One epoch over ds: make_order(ds.count, batch, seed, epoch, pad, flip) -- the last partial
        batch dropped -- set as ds's order (one device synchronisation), then every step enqueued.
        rrc (a dict with `scale` and / or `ratio`, may be empty; needs pad == 0): the order is
        make_rrc_order's instead, a random-resized crop of every stored image to ds's output size.
        update_bits (as set_update_bits takes): set on the stream ahead of the epoch's steps.
        Returns the number of steps; asynchronous."""
        from .dataset import make_order, make_rrc_order
        if update_bits is not None:
            self.set_update_bits(update_bits, stream)
        if rrc is not None:
            if pad != 0:
                raise ValueError("rrc needs pad == 0")
            if set(rrc) - {"scale", "ratio"}:
                raise ValueError("rrc takes scale and ratio")
            index, xform, windows = make_rrc_order(ds.count, self.batch, seed, epoch, ds.h, ds.w, flip=flip,
                                                   drop_last=True, **rrc)
            ds.set_order(index, xform, windows)
        else:
            index, xform = make_order(ds.count, self.batch, seed, epoch, pad=pad, flip=flip, drop_last=True)
            ds.set_order(index, xform if (pad or flip) else None)
        steps = len(index) // self.batch
        self.train_steps(ds, 0, steps, stream)
        return steps

    def evaluate_dataset(self, ds, stream=None, windows=None) -> dict:
        """evaluate() on a DeviceDataset: a sequential order (which replaces ds's), the last partial
        batch padded with -1 entries, the totals reset, every batch enqueued, one synchronisation in
        eval_read.  windows: int32 [ds.count][4], one crop per image; when none are given and ds's
        stored size is not its output size, center_windows(ds.count, ds.h, ds.w)."""
        from .dataset import center_windows
        n, b = ds.count, self.batch
        pad = (-n) % b
        index = np.concatenate([np.arange(n, dtype=np.int32), np.full(pad, -1, np.int32)])
        if windows is None and (ds.h, ds.w) != (ds.oh, ds.ow):
            windows = center_windows(n, ds.h, ds.w)
        if windows is not None:
            windows = np.asarray(windows, np.int32).reshape(n, 4)
            windows = np.concatenate([windows, np.tile(np.array([0, 0, 1, 1], np.int32), (pad, 1))])
        ds.set_order(index, None, windows)
        self.eval_reset(stream)
        self.eval_steps(ds, 0, len(index) // b, stream)
        return self.eval_read(stream)

    def train_metrics(self, enable: bool):
        """Add each dataset training step's loss / top-1 / top-k (of the step's own logits and
        labels) to running totals on the device (default off: nothing is launched)."""
        check(self._lib.niti_model_train_metrics(self._h, 1 if enable else 0), "train_metrics")

    def train_metrics_reset(self, stream=None):
        check(self._lib.niti_model_train_metrics_reset(self._h, _stream(stream)), "train_metrics_reset")

    def train_metrics_read(self, stream=None) -> dict:
        """The training totals (synchronises), in eval_read's form."""
        t = L.EvalTotals()
        check(self._lib.niti_model_train_metrics_read(self._h, C.byref(t), _stream(stream)), "train_metrics_read")
        return self._totals_dict(t)

    def input(self, stream=None):
        """The last step's quantised input x (NCHW int8) and its exponent."""
        l0 = self.layers[0]
        out = np.empty((self.batch, l0["c_in"], l0["h"], l0["w"]), np.int8)
        e = C.c_int()
        check(self._lib.niti_model_get_input(self._h, out.ctypes.data_as(C.c_void_p), C.byref(e), _stream(stream)),
              "get_input")
        return out, int(e.value)

    def logits(self, stream=None):
        last = self.layers[-1]
        out = np.empty((self.batch, last["c_out"]), np.int8)
        e = C.c_int()
        check(self._lib.niti_model_get_logits(self._h, out.ctypes.data_as(C.c_void_p), C.byref(e),
                                              _stream(stream)), "get_logits")
        return out, int(e.value)

    def tap(self, i, which, stream=None):
        l = self.layers[i]
        if which == 1:
            shape = self.weight_shape(i)
        else:
            shape = (self.batch, l["c_out"], l["oh"], l["ow"])
        out = np.empty(shape, np.int8)
        check(self._lib.niti_model_get_tap(self._h, i, which, out.ctypes.data_as(C.c_void_p), out.nbytes,
                                           _stream(stream)), "get_tap")
        return out

    def autotune(self, reps: int = 5, stream=None):
        """Time candidate GEMM plans per layer phase and keep the fastest (niti_model_autotune).
        Call after one train_step; plans never change results."""
        check(self._lib.niti_model_autotune(self._h, int(reps), _stream(stream)), "autotune")

    def plan(self, layer: int, phase: int):
        """(bm, bn, splits, strategy) of one layer phase; 32x32 = the tap-sharing weight gradient,
        16x16 = the P16 weight gradient."""
        info = (C.c_int * 4)()
        check(self._lib.niti_model_plan_info(self._h, layer, phase, info), "plan_info")
        return tuple(info)

    def plans(self):
        """{(layer, phase): (bm, bn, splits, strategy)}; phase 0 fwd / 1 input grad / 2 weight grad,
        strategy 0 store / 1 recompute / 2 split-K / 3 the speculative pair / 4 fused: one launch with the
        rescale behind an in-kernel grid barrier (forward / input gradient).  A depthwise layer has
        no GEMM plan and no entry."""
        out = {}
        for i in range(len(self.layers)):
            for ph in (0, 1, 2):
                if (ph == 1 and i == 0) or self.layers[i]["depthwise"]:
                    continue
                out[(i, ph)] = self.plan(i, ph)
        return out

    def set_plan(self, layer: int, phase: int, plan=None):
        """Force (bm, bn, splits, strategy) for one layer phase; None restores the default."""
        arr = None if plan is None else (C.c_int * 4)(*[int(v) for v in plan])
        check(self._lib.niti_model_plan_set(self._h, layer, phase, arr), "plan_set")

    @staticmethod
    def reset_plans():
        """Drop every plan override in this process."""
        L.lib().niti_plan_reset()

    def set_overlap(self, enable: bool):
        """Weight gradients on a second stream overlapping the input gradients (default on)."""
        check(self._lib.niti_model_set_overlap(self._h, int(enable)), "set_overlap")

    def set_graph(self, enable: bool):
        """Replay the step as a hipGraph or launch its kernels directly (default)."""
        check(self._lib.niti_model_set_graph(self._h, int(enable)), "set_graph")

    def keep_grads(self, enable: bool):
        """Store each step's int8 weight gradient for tap(layer, 1) (default) or not: the SGD
        kernel then updates the weights without writing the copy."""
        check(self._lib.niti_model_keep_grads(self._h, int(enable)), "keep_grads")

    def set_rowconv(self, enable: bool):
        """Forward convs and input gradients of the stride-1 pad-1 3x3 layers on the register-fed
        kernel with the fused rescale (default) or on the GEMM + requantisation passes; identical
        results."""
        check(self._lib.niti_model_set_rowconv(self._h, int(enable)), "set_rowconv")

    def rowconv_error(self) -> int:
        """1 if an in-kernel grid barrier of the register-fed forward ever timed out."""
        return int(self._lib.niti_model_rowconv_error(self._h))

    def spec_stats(self):
        """Per layer: (fwd hint, fwd launches redone, fwd pairs stored, dgrad hint, dgrad redone,
        dgrad stored) of the speculative row-kernel pairs (niti_model_spec_stats)."""
        n = len(self.layers)
        buf = (C.c_uint32 * (6 * n))()
        check(self._lib.niti_model_spec_stats(self._h, buf, n), "spec_stats")
        return [tuple(buf[6 * i:6 * i + 6]) for i in range(n)]

    def set_probe(self, layer: int, phase: int, max_launches: int = 256):
        check(self._lib.niti_model_set_probe(self._h, layer, phase, max_launches), "set_probe")

    def spec_slot(self, layer: int, dgrad: int):
        """The 32 words of one row-kernel layer's speculative slot (diagnostics)."""
        out = (C.c_uint32 * 32)()
        check(self._lib.niti_model_spec_slot(self._h, int(layer), int(dgrad), out), "spec_slot")
        return list(out)

    def probe_pause(self, paused: bool):
        """Skip (True) or time again (False) the armed probe's launches; host-side only."""
        check(self._lib.niti_model_probe_pause(self._h, 1 if paused else 0), "probe_pause")

    def probe_read(self):
        t = C.c_double()
        n = C.c_int()
        check(self._lib.niti_model_probe_read(self._h, C.byref(t), C.byref(n)), "probe_read")
        return float(t.value), int(n.value)

    def run_phase(self, layer: int, phase: int, stream=None):
        """One layer phase of the last step again (0 fwd, 1 input grad, 2 weight grad), alone."""
        check(self._lib.niti_model_run_phase(self._h, int(layer), int(phase), _stream(stream)), "run_phase")

    def probe_read_span(self):
        """(summed ms, launches) of the weight-gradient probe's in-kernel spans (device wall clock)."""
        t, n = C.c_double(0), C.c_int(0)
        check(self._lib.niti_model_probe_read_span(self._h, C.byref(t), C.byref(n)), "probe_read_span")
        return t.value, n.value

    def step_macs(self) -> int:
        return int(self._lib.niti_model_step_macs(self._h))

    def attach_comm(self, unique_id: bytes, rank: int, world: int, exact: bool = True):
        check(self._lib.niti_model_attach_comm(self._h, unique_id, rank, world, 1 if exact else 0), "attach_comm")

    def attach_local(self, group: "LocalGroup", rank: int, exact: bool = True):
        """Join an in-process rank group on this device (one host thread per rank)."""
        check(self._lib.niti_model_attach_local(self._h, group._h, rank, 1 if exact else 0), "attach_local")
        self._group = group  # keep the group alive as long as the model

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        check(L.lib().niti_dp_get_unique_id(buf), "unique_id")
        return buf.raw

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.niti_model_destroy(h)
            self._h = None


class LocalGroup:
    """niti_local_group: `world` ranks of the data-parallel protocol on ONE device, one host
    thread per rank, collectives reduced on the device (include/niti_hip.h)."""

    def __init__(self, world: int):
        self._lib = L.lib()
        h = C.c_void_p()
        check(self._lib.niti_local_group_create(int(world), C.byref(h)), "local_group_create")
        self._h = h
        self.world = world

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.niti_local_group_destroy(h)
            self._h = None
