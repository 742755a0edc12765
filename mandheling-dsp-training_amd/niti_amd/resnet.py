"""User-defined residual networks: a model from a stage list (niti_resnet_spec, include/niti_hip.h).

A spec is a dict (or keywords) with
    depths   the basic blocks per stage, e.g. (3, 4, 6, 3) for ResNet-34 or (3, 3, 3) for ResNet-20
    width    the first stage's channels (stage s has width << s; default 64)
    classes  the head's class count
    in_c     the input channels (default 3)
    stem     "imagenet": conv 7x7 / 2 pad 3 + the 3x3 / 2 max pool (the default); "cifar": conv
             3x3 / 1 pad 1, no pool; or a tuple (kernel, stride, pad, pool)
The layer order, the projection rule and what is refused are the header's.
"""
from __future__ import annotations

import ctypes as C

from . import _lib as L
from ._lib import check

STEMS = {"imagenet": (7, 2, 3, 1), "cifar": (3, 1, 1, 0)}
_KEYS = ("in_c", "stem", "width", "depths", "classes")


def normalize_resnet_spec(spec=None, **kw) -> dict:
    """The spec as a dict of plain ints -- in_c, stem [kernel, stride, pad, pool], width, depths
    (a list), classes -- which is what snapshots store and compare.  Only the form is checked here
    (ValueError); the values are the library's to refuse."""
    d = dict(spec or {})
    d.update(kw)
    extra = set(d) - set(_KEYS)
    if extra or "depths" not in d or "classes" not in d:
        raise ValueError(f"a residual spec needs depths and classes, takes {_KEYS}, got {sorted(d)}")
    stem = d.get("stem", "imagenet")
    if isinstance(stem, str):
        if stem not in STEMS:
            raise ValueError(f"stem {stem!r}: one of {sorted(STEMS)} or a tuple (kernel, stride, pad, pool)")
        stem = STEMS[stem]
    stem = tuple(stem)
    if len(stem) != 4:
        raise ValueError(f"stem: a tuple (kernel, stride, pad, pool), got {stem!r}")
    if isinstance(d["depths"], int):
        raise ValueError("depths: the blocks per stage as a sequence")
    depths = [int(x) for x in d["depths"]]
    if not 1 <= len(depths) <= L.RESNET_MAX_STAGES:
        raise ValueError(f"depths: 1 to {L.RESNET_MAX_STAGES} stages, got {len(depths)}")
    k, s, p, pool = (int(x) for x in stem)
    return {"in_c": int(d.get("in_c", 3)), "stem": [k, s, p, 1 if pool else 0], "width": int(d.get("width", 64)),
            "depths": depths, "classes": int(d["classes"])}


def to_c(spec: dict) -> L.ResnetSpec:
    """The niti_resnet_spec of a normalised spec."""
    cs = L.ResnetSpec()
    cs.in_c, cs.width, cs.classes = spec["in_c"], spec["width"], spec["classes"]
    cs.stem_kernel, cs.stem_stride, cs.stem_pad, cs.stem_pool = spec["stem"]
    cs.n_stages = len(spec["depths"])
    for i, dep in enumerate(spec["depths"]):
        cs.depths[i] = dep
    return cs


def resnet_layers(spec=None, in_hw: int = 0, **kw) -> list:
    """The derived parameter layers of a spec over in_hw x in_hw inputs, as dicts with the oracle's
    keys name, ci, co, k, stride, pad, h (host only: niti_model_resnet_check); names as
    oracle/niti_resnet_ref.py resnet18_convs gives them (conv1, layer<stage>.<block>.a / .b / .proj,
    fc).  ValueError for a malformed spec, NitiError (NOT_SUPPORT) for one the library does not run."""
    spec = normalize_resnet_spec(spec, **kw)
    cs = to_c(spec)
    n = C.c_int(0)
    shapes = ((C.c_int * 8) * L.RESNET_MAX_LAYERS)()
    code = L.lib().niti_model_resnet_check(C.byref(cs), int(in_hw), C.byref(n), shapes)
    if code == L.INVALID_VALUE:
        raise ValueError(f"malformed residual network for a {in_hw} x {in_hw} input: {spec}")
    check(code, "resnet_check")
    names = ["conv1"]
    for stage, dep in enumerate(spec["depths"]):
        for blk in range(dep):
            names += [f"layer{stage + 1}.{blk}.a", f"layer{stage + 1}.{blk}.b"]
            if stage > 0 and blk == 0:
                names.append(f"layer{stage + 1}.{blk}.proj")
    names.append("fc")
    assert len(names) == n.value, (len(names), n.value)
    return [dict(name=nm, ci=s[0], co=s[1], k=s[2], stride=s[3], pad=s[4], h=s[5]) for nm, s in zip(names, shapes)]
