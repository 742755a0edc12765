"""Parameter snapshots for the NITI step.

The reference snapshots the trainable Variables with `Variable::save(model->parameters(), path)`
at the end of each epoch (`EE/tools/train/source/demo/mnistTrain.cpp:375-376`); the NITI
weights are int8 OIHW tensors whose power-of-two scale `wscale` lives beside them as a
fixed int8 chosen at init (`EE/tools/train/source/nn/NN.cpp:1108-1134`, never updated by
NITI_SGD, `NITI_SGD.hpp:20-54`).  A snapshot here holds exactly that state:

    layer{i}.weight  int8 [C_out, C_in, KH, KW]  (OIHW, the reference's parameter layout)
    layer{i}.wscale  int8 [1]                    (the side-car the MNN file does not carry)

stored as safetensors (no code executes on load) with `arch` / `num_layers` metadata; the snapshot
of a user-defined chain network (arch ARCH_CHAIN) also carries its layer list and input as one
JSON string under the metadata key `chain` (`load_chain`), that of a user-defined residual network
(arch ARCH_RESNET) its stage list and input size under `resnet` (`load_resnet`).  The
MNN flatbuffer container itself is not reproduced: `Variable::load` of that format needs
the MNN schema, which is outside the hot path; the tensors and their order are the same.
"""
from __future__ import annotations

import json

import numpy as np
from safetensors.numpy import load_file, save_file

FORMAT = "niti-int8-params-v1"


def chain_record(spec, in_c: int, in_hw: int) -> dict:
    """What a chain model's snapshot stores about its network (compared as a whole on load)."""
    from .chain import normalize_spec
    return {"spec": normalize_spec(spec), "in_c": int(in_c), "in_hw": int(in_hw)}


def resnet_record(spec, in_hw: int) -> dict:
    """What a stage-list model's snapshot stores about its network (compared as a whole on load)."""
    from .resnet import normalize_resnet_spec
    return {"spec": normalize_resnet_spec(spec), "in_hw": int(in_hw)}


def save_params(path: str, weights, wscales, arch: int, in_hw: int = 0, chain: dict | None = None,
                resnet: dict | None = None, update_bits=None) -> None:
    """Write per-layer int8 OIHW weights and their int8 wscale side-car.  chain: a chain_record()
    for a user-defined chain, resnet: a resnet_record() for a user-defined residual network (both
    None: the file is a built-in network's, as it always was).  update_bits: the model's per-layer
    update bits, recorded (metadata key `update_bits`) only when some layer differs from 2."""
    if len(weights) != len(wscales):
        raise ValueError(f"{len(weights)} weights but {len(wscales)} wscales")
    tensors = {}
    for i, (w, s) in enumerate(zip(weights, wscales)):
        w = np.asarray(w)
        if w.dtype != np.int8 or w.ndim != 4:
            raise ValueError(f"layer {i}: expected int8 OIHW weight, got {w.dtype} {w.shape}")
        if not -128 <= int(s) <= 127:
            raise ValueError(f"layer {i}: wscale {s} does not fit int8")
        tensors[f"layer{i}.weight"] = np.ascontiguousarray(w)
        tensors[f"layer{i}.wscale"] = np.array([int(s)], np.int8)
    meta = {"format": FORMAT, "arch": str(int(arch)), "num_layers": str(len(weights)), "in_hw": str(int(in_hw))}
    if chain is not None:
        meta["chain"] = json.dumps(chain, sort_keys=True)
    if resnet is not None:
        meta["resnet"] = json.dumps(resnet, sort_keys=True)
    if update_bits is not None and any(int(b) != 2 for b in update_bits):
        meta["update_bits"] = json.dumps([int(b) for b in update_bits])
    save_file(tensors, path, metadata=meta)


def expect_chain(found, record, path: str) -> None:
    """Refuse (ValueError) a snapshot whose chain (or resnet) record `found` is not the model's
    `record`; a built-in model (record None) takes any snapshot its arch check let through."""
    if record is not None and found != record:
        raise ValueError(f"{path}: the snapshot's layer list {found} differs from the model's {record}")


def load_chain(path: str):
    """The chain_record() a snapshot carries, or None (a built-in network's snapshot)."""
    from safetensors import safe_open

    with safe_open(path, framework="numpy") as f:
        meta = f.metadata() or {}
    if meta.get("format") != FORMAT:
        raise ValueError(f"{path}: not a {FORMAT} snapshot (format={meta.get('format')!r})")
    if "chain" not in meta:
        return None
    try:
        rec = json.loads(meta["chain"])
        return chain_record(rec["spec"], rec["in_c"], rec["in_hw"])
    except (ValueError, KeyError, TypeError) as e:
        raise ValueError(f"{path}: malformed chain record ({e!r})") from None


def load_resnet(path: str):
    """The resnet_record() a snapshot carries, or None."""
    from safetensors import safe_open

    with safe_open(path, framework="numpy") as f:
        meta = f.metadata() or {}
    if meta.get("format") != FORMAT:
        raise ValueError(f"{path}: not a {FORMAT} snapshot (format={meta.get('format')!r})")
    if "resnet" not in meta:
        return None
    try:
        rec = json.loads(meta["resnet"])
        return resnet_record(rec["spec"], rec["in_hw"])
    except (ValueError, KeyError, TypeError) as e:
        raise ValueError(f"{path}: malformed resnet record ({e!r})") from None


def check_update_bits(bits, n_layers: int, path: str):
    """The `update_bits` record of a snapshot as a list of n_layers ints in 0..7 (ValueError
    otherwise); None stays None."""
    if bits is None:
        return None
    try:
        bits = [int(b) for b in bits]
    except (ValueError, TypeError) as e:
        raise ValueError(f"{path}: malformed update_bits ({e!r})") from None
    if len(bits) != n_layers or any(not 0 <= b <= 7 for b in bits):
        raise ValueError(f"{path}: update_bits {bits} for a model of {n_layers} layers (one value in 0..7 each)")
    return bits


def load_update_bits(path: str):
    """The update bits a snapshot carries (a list), or None: a snapshot of a model at the default."""
    from safetensors import safe_open

    with safe_open(path, framework="numpy") as f:
        meta = f.metadata() or {}
    if "update_bits" not in meta:
        return None
    try:
        return list(json.loads(meta["update_bits"]))
    except (ValueError, TypeError) as e:
        raise ValueError(f"{path}: malformed update_bits ({e!r})") from None


def load_params(path: str):
    """Read a snapshot back: (weights, wscales, arch).  Raises ValueError on a malformed file."""
    from safetensors import safe_open

    with safe_open(path, framework="numpy") as f:
        meta = f.metadata() or {}
    if meta.get("format") != FORMAT:
        raise ValueError(f"{path}: not a {FORMAT} snapshot (format={meta.get('format')!r})")
    try:
        n = int(meta["num_layers"])
        arch = int(meta["arch"])
    except (KeyError, ValueError, TypeError) as e:
        raise ValueError(f"{path}: malformed snapshot metadata ({e!r})") from None
    if n <= 0:
        raise ValueError(f"{path}: num_layers {n}")
    t = load_file(path)
    weights, wscales = [], []
    for i in range(n):
        w, s = t.get(f"layer{i}.weight"), t.get(f"layer{i}.wscale")
        if w is None or s is None or w.dtype != np.int8 or s.dtype != np.int8 or s.shape != (1,):
            raise ValueError(f"{path}: layer {i} missing or malformed")
        weights.append(w)
        wscales.append(int(s[0]))
    return weights, wscales, arch
