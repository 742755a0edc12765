"""User-defined chain networks: a model from a layer list (niti_chain_layer3, include/niti_hip.h).

A spec is a list of layers, each a dict with the keys c_out, kernel and optionally pad, relu,
pool, flatten, depthwise (default 0), stride (default 1; 1 or 2), skip (default 0), gpool (default 0: 1 sums
the layer's map into a 1x1 map, the global sum pool), or a tuple (c_out, kernel, pad, relu,
pool, flatten, depthwise, stride, skip, gpool) whose tail may be left out.  The input channels and map size of every layer are derived;
the last layer's c_out is the class count.  A depthwise layer has its input's channels: its c_out
may be 0 or, in a dict, left out.
"""
from __future__ import annotations

import ctypes as C

from . import _lib as L
from ._lib import check

_KEYS = ("c_out", "kernel", "pad", "relu", "pool", "flatten", "depthwise", "stride", "skip", "gpool")
_OLD_MAX_LAYERS = 24  # what the entry points before niti_model_chain_check4 / _create_chain4 take
_DEFAULT = {"stride": 1}


def normalize_spec(spec) -> list:
    """The spec as a list of dicts of plain ints (what snapshots store and compare): the keys c_out,
    kernel, pad, relu, pool, flatten and, only for a list that has a depthwise layer, depthwise, only
    for a list that has a layer of stride other than 1, stride, only for a list that has a skip, skip, only
    for a list that has a global pool, gpool -- so the record of a list without one is what it always was.  A depthwise layer's c_out of 0 becomes
    the previous layer's c_out where that is the layer's input (not after a flatten, not layer 0:
    lists the check refuses anyway)."""
    out = []
    for i, l in enumerate(spec):
        if isinstance(l, dict):
            extra = set(l) - set(_KEYS)
            dw = bool(l.get("depthwise", 0))
            if extra or ("c_out" not in l and not dw) or "kernel" not in l:
                raise ValueError(f"layer {i}: needs c_out and kernel, takes {_KEYS}, got {sorted(l)}")
            d = {k: int(l.get(k, _DEFAULT.get(k, 0))) for k in _KEYS}
        else:
            l = tuple(l)
            if not 2 <= len(l) <= len(_KEYS):
                raise ValueError(
                    f"layer {i}: a tuple (c_out, kernel[, pad, relu, pool, flatten, depthwise, stride, skip, gpool]), got {l!r}")
            d = {k: int(l[j]) if j < len(l) else _DEFAULT.get(k, 0) for j, k in enumerate(_KEYS)}
        for k in ("relu", "pool", "flatten"):
            d[k] = 1 if d[k] else 0
        if d["stride"] < 1:
            raise ValueError(f"layer {i}: stride {d['stride']}")
        if d["depthwise"] == 1 and d["c_out"] == 0 and out and not out[-1]["flatten"]:
            d["c_out"] = out[-1]["c_out"]
        out.append(d)
    if not out:
        raise ValueError("an empty layer list")
    if not any(d["depthwise"] for d in out):
        for d in out:
            del d["depthwise"]
    if all(d["stride"] == 1 for d in out):
        for d in out:
            del d["stride"]
    for k in ("skip", "gpool"):
        if all(d[k] == 0 for d in out):
            for d in out:
                del d[k]
    return out


def strided(spec) -> bool:
    """A normalised spec that has a layer of stride other than 1: it goes through the `3` entry points
    (niti_model_chain_check3 / _create_chain3), every other list through the ones it always went through."""
    return any("stride" in d for d in spec)


def wide(spec) -> bool:
    """A normalised spec that has a skip or a global pool, or more than 24 layers: it goes through the `4`
    entry points (niti_model_chain_check4 / _create_chain4), every other list where it always went."""
    return any("skip" in d or "gpool" in d for d in spec) or len(spec) > _OLD_MAX_LAYERS


def entry_points(spec):
    """(check, create) -- the C entry points a normalised spec goes through."""
    lib = L.lib()
    if wide(spec):
        return lib.niti_model_chain_check4, lib.niti_model_create_chain4
    if strided(spec):
        return lib.niti_model_chain_check3, lib.niti_model_create_chain3
    return lib.niti_model_chain_check2, lib.niti_model_create_chain2


def to_c(spec):
    """(niti_chain_layer2 array -- niti_chain_layer3 for a wide() spec --, count) of a normalised spec."""
    w = wide(spec)
    arr = ((L.ChainLayer3 if w else L.ChainLayer2) * len(spec))()
    for a, d in zip(arr, spec):
        a.c_out, a.kernel, a.stride, a.pad = d["c_out"], d["kernel"], d.get("stride", 1), d["pad"]
        a.relu, a.pool, a.flatten = d["relu"], d["pool"], d["flatten"]
        a.depthwise = d.get("depthwise", 0)
        if w:
            a.skip, a.gpool = d.get("skip", 0), d.get("gpool", 0)
    return arr, len(spec)


def chain_layers(spec, in_c: int, in_hw: int) -> list:
    """The derived layer list of a spec over in_c x in_hw x in_hw inputs, as dicts with the keys
    ci, co, k, pad, h, relu, pool, flatten and, for a list that has a depthwise layer, depthwise, for a
    list that has a strided layer, stride, for a list that has a skip, skip, for a list that has a global
    pool, gpool (host only: niti_model_chain_check2, _check3 for a list with a strided layer, _check4 for a
    wide() list).  ValueError for a malformed spec, NitiError (NOT_SUPPORT) for one
    the library does not run."""
    spec = normalize_spec(spec)
    arr, n = to_c(spec)
    shapes = ((C.c_int * 8) * n)()
    fn = entry_points(spec)[0]
    code = fn(arr, n, int(in_c), int(in_hw), shapes)
    if code == L.INVALID_VALUE:
        raise ValueError(f"malformed layer list for a {in_c} x {in_hw} x {in_hw} input: {spec}")
    check(code, "chain_check")
    out = [dict(ci=s[0], co=s[1], k=s[2], pad=s[3], h=s[4], relu=d["relu"], pool=d["pool"], flatten=d["flatten"])
           for s, d in zip(shapes, spec)]
    for o, d in zip(out, spec):  # (the list of a spec without such a layer is what it always was)
        if "depthwise" in d:
            o["depthwise"] = d["depthwise"]
        if "stride" in d:
            o["stride"] = d["stride"]
        for k in ("skip", "gpool"):
            if k in d:
                o[k] = d[k]
    return out
