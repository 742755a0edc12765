"""Starting weights for a NITI model: the reference's int8 Xavier initialiser.

The reference fills every NITI conv weight with `NITIXavier` (nn/Initializer.cpp:118-134):
normal draws of std = sqrt(2 / (fan_in + fan_out)), fan_in = C_in * KH * KW, fan_out = C_out * KH * KW,
turned into int8 by `Distributions::niti_normal_int8` (nn/Distributions.cpp:26-51): range = max |t|,
w = round(t / range * 127), wscale = ceil(log2f(range)) - 7.  The reference seeds its engine from
the clock; here the caller supplies a numpy Generator, so a run can be repeated.
"""
from __future__ import annotations

import numpy as np


def xavier_int8(shape, rng: np.random.Generator):
    """(w int8 OIHW of `shape`, wscale) drawn from `rng`."""
    shape = tuple(int(d) for d in shape)
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError(f"an OIHW shape of four positive sizes, got {shape}")
    fan_in = shape[1] * shape[2] * shape[3]
    fan_out = shape[0] * shape[2] * shape[3]
    std = np.sqrt(2.0 / (fan_in + fan_out))
    t = rng.normal(0.0, std, size=shape).astype(np.float32)
    span = float(np.abs(t).max())
    wscale = int(np.ceil(np.log2(span))) - 7
    return np.round(t / span * 127).astype(np.int8), wscale
