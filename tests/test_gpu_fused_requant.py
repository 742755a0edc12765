"""The fused forms of the requantisation pass and the stem pool pair against the CPU oracle, bit
for bit, through the split device API (niti_amd.ops over niti_requant_act_fused, niti_maxpool_arg
and niti_maxpool_grad_arg): kernels the training step otherwise reaches alone.

Cases, references and what each case guards: tests/fused_requant_cases.py (its tables are checked
on the CPU by tests/test_fused_requant_cases.py).  Every output buffer is pre-filled with 77
between two guard runs and compared whole with np.array_equal against the oracle or numpy; the
GPU-vs-GPU assertions are the named second ones."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fused_requant_cases as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = [pin for _, pin in F.PINS]


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401  (fails loudly without the HIP library)
    return torch


@pytest.fixture(scope="module")
def ops(T):
    from niti_amd import ops
    return ops


def _sid(shape):
    return "x".join(str(int(v)) for v in shape)


WRAP_EXP = (F.WRAP["exp_in"], F.WRAP["wscale"])


# --------------------------------------------------------------------------------- A. pool forward
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", F.PF_SHAPES, ids=_sid)
def test_pool_forward(T, ops, shape, relu):
    """requant_quad_kernel<RQ_POOL_FWD>: the pre-pool output and the 2x2 window max on every pinned
    range."""
    bad = [b for pin in PINS for b in F.run_pool_fwd(T, ops, shape, pin, relu)]
    assert not bad, bad


def test_pool_forward_second_pass(T, ops):
    """2,097,456 units: 304 more than the grid's four loads per thread."""
    bad = F.run_pool_fwd(T, ops, F.PF_BIG, F.BIG_PIN, True)
    assert not bad, bad


def test_pool_forward_exponent_wraps(T, ops):
    bad = F.run_pool_fwd(T, ops, F.PF_WRAP_SHAPE, F.WRAP["pin"], False, WRAP_EXP)
    assert not bad, bad


# --------------------------------------------------------------------------------- B. pool backward
@pytest.mark.parametrize("with_out", [True, False], ids=["out", "noout"])
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("geo", F.PB_SHAPES, ids=_sid)
def test_pool_backward(T, ops, geo, relu, with_out):
    """requant_quad_kernel<RQ_POOL_BWD>: dx (first max wins, the relu gradient), its C32 copy and the
    optional requantised dy."""
    bad = [b for pin in PINS for b in F.run_pool_bwd(T, ops, geo[:4], pin, relu, with_out, c32=geo[4])]
    assert not bad, bad


def test_pool_backward_second_pass(T, ops):
    bad = F.run_pool_bwd(T, ops, F.PB_BIG[:4], F.BIG_PIN, True, True)
    assert not bad, bad


def test_pool_backward_exponent_wraps(T, ops):
    geo = F.PB_WRAP_SHAPE
    bad = F.run_pool_bwd(T, ops, geo[:4], F.WRAP["pin"], True, True, c32=geo[4], exp=WRAP_EXP)
    assert not bad, bad


# --------------------------------------------------------------------------------- C. P16 plain
@pytest.mark.parametrize("shape", F.P16_SHAPES, ids=_sid)
def test_p16_plain(T, ops, shape):
    """requant_p16_plain_kernel: the NHWC16 output and its P16 copy, relu off / on and with the
    relu-gradient mask."""
    bad = [b for pin in PINS for b in F.run_p16_plain(T, ops, *shape, pin)]
    assert not bad, bad


def test_p16_plain_grid_stride(T, ops):
    bad = F.run_p16_plain(T, ops, *F.P16_BIG, F.BIG_PIN, modes=F.P16_MODES[2:])
    assert not bad, bad


def test_p16_plain_exponent_wraps(T, ops):
    bad = F.run_p16_plain(T, ops, *F.P16_WRAP_SHAPE, F.WRAP["pin"], exp=WRAP_EXP)
    assert not bad, bad


# --------------------------------------------------------------------------------- D. P16 pool backward
@pytest.mark.parametrize("geo", F.P16B_SHAPES, ids=_sid)
def test_p16_pool_backward(T, ops, geo):
    """requant_p16_kernel<RQ_POOL_BWD, W>, W = 2 / 4 / 8 / 16: dx, its P16 copy and the optional
    requantised dy, pool relu off and on."""
    n, w, ldc = geo
    bad = [b for pin in PINS for relu in (False, True) for with_out in (True, False)
           for b in F.run_pool_bwd(T, ops, (n, w, w, ldc), pin, relu, with_out, p16=True)]
    assert not bad, bad


def test_p16_pool_backward_exponent_wraps(T, ops):
    bad = F.run_pool_bwd(T, ops, (3, 4, 4, 48), F.WRAP["pin"], True, True, p16=True, exp=WRAP_EXP)
    assert not bad, bad


# --------------------------------------------------------------------------------- E. zero_cls
@pytest.mark.parametrize("with_mask", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("shape", F.ZC_SHAPES, ids=_sid)
def test_zero_cls(T, ops, shape, with_mask):
    """The plain pass with every class mask 1 .. 14: 0 in the skipped classes, whose accumulators
    hold 0x7fffffff / INT32_MIN, the rule's value elsewhere."""
    bad = [b for cls in F.ZC_MASKS for pin in PINS for b in F.run_zero_cls(T, ops, shape, cls, pin, with_mask)]
    assert not bad, bad


def test_zero_cls_exponent_wraps(T, ops):
    bad = F.run_zero_cls(T, ops, F.ZC_WRAP_SHAPE, 6, F.WRAP["pin"], True, WRAP_EXP)
    assert not bad, bad


# --------------------------------------------------------------------------------- F. 3x3 / 2 pool
@pytest.mark.parametrize("with_pre", [True, False], ids=["pre", "nopre"])
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("shape", F.P3_SHAPES, ids=_sid)
def test_pool3(T, ops, shape, relu, with_pre):
    """requant_pool3_kernel<RELU>: the pooled image, the first-max positions, the optional pre-pool
    output and exp_out, odd and even sides, one to three strips."""
    bad = [b for pin in PINS for b in F.run_pool3(T, ops, shape, pin, relu, with_pre)]
    assert not bad, bad


def test_pool3_exponent_wraps(T, ops):
    bad = F.run_pool3(T, ops, F.P3_WRAP_SHAPE, F.WRAP["pin"], True, True, WRAP_EXP)
    assert not bad, bad


_CHILD = """
import sys
sys.path[:0] = {paths!r}
import torch
import fused_requant_cases as F
from niti_amd import ops
bad, runs = F.pool3_table_mismatch(torch, ops, F.P3_CHILD_SHAPES)
torch.cuda.synchronize()
for b in bad:
    print("MISMATCH", b)
print("checked", runs, "mismatches", len(bad))
sys.exit(1 if bad else 0)
"""


@pytest.mark.parametrize("env", F.P3_CHILD_ENVS, ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_pool3_strip_settings(T, env):
    """NITI_RQ3_ROWS = 1 / 3 and NITI_RQ3_REMAP = 1 (each read once per process, so a fresh child):
    the 3 x 7 x 9 x 48 and 1 x 17 x 12 x 32 cases on every pinned range."""
    paths = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"),
             os.path.join(ROOT, "mandheling-dsp-training_amd")]
    r = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert f"checked {len(F.P3_CHILD_SHAPES) * len(PINS) * 4} mismatches 0" in r.stdout


# --------------------------------------------------------------------------------- G. stem pool pair
PP_GEOS = [(*m, cp) for m in F.PP_MAPS for cp in F.PP_CPS]


@pytest.mark.parametrize("pool", F.PP_POOLS, ids=_sid)
@pytest.mark.parametrize("geo", PP_GEOS, ids=_sid)
def test_maxpool_arg(T, ops, geo, pool):
    """niti_maxpool_arg: y against the oracle's pool and arg against the position its pool gradient
    routes to (the first in-image element equal to the window max; on the 1 x 1 and 2 x 2 maps
    under a 3 x 3 window, see fused_requant_cases.first_at_least); second assertion: y is
    niti_maxpool's."""
    n, h, w, cp = geo
    k, s, p = pool
    bad = []
    for relu in (False, True):
        c = F.pp_case(n, h, w, cp, k, s, p, relu)
        tag = ("G", geo, pool, relu)
        x = F.dev(T, c["x"])
        y, arg = F.Buf(T, c["y"].shape), F.Buf(T, c["arg"].shape)
        ops.maxpool_arg(x, k, s, p, y=y.t, arg=arg.t, ohw=c["y"].shape[1:3])
        y.check(c["y"], "y", bad, tag)
        arg.check(c["arg"], "arg", bad, tag)
        assert T.equal(y.t, ops.maxpool(x, k, s, p, ohw=c["y"].shape[1:3])), tag
    assert not bad, bad


@pytest.mark.parametrize("shape", F.PP_SHARED_WITH_F, ids=_sid)
def test_maxpool_arg_equals_pool3_arg(T, ops, shape):
    """On the fused stem pass's relu output, niti_maxpool_arg gives the positions group F expects of
    requant_pool3_kernel, and the same pooled image on maps of at least 3 x 3 (below that the
    reference pool clips its window and the fused pass, which has no reference counterpart there,
    does not)."""
    n, h, w, ldc = shape
    bad = []
    for pin in PINS:
        c = F.p3_case(shape, pin, True)
        y, arg = F.Buf(T, c["out"].shape), F.Buf(T, c["arg"].shape)
        ops.maxpool_arg(F.dev(T, c["pre"]), 3, 2, 1, y=y.t, arg=arg.t, ohw=c["out"].shape[1:3])
        if min(h, w) >= 3:
            y.check(c["out"], "y", bad, ("G/F", shape, pin))
        arg.check(c["arg"], "arg", bad, ("G/F", shape, pin))
    assert not bad, bad


def _grad_forms(T, ops, c, h, w, pool, tag, bad):
    """niti_maxpool_grad_arg without relu, with relu from x and with relu from `pooled`, each against
    the reference (arg is the reference's: an input here)."""
    k, s, p = pool
    arg, dy, x, pooled = (F.dev(T, c[key]) for key in ("arg", "dy", "x", "pooled"))
    plain = c["sums"].astype(np.int8)   # the int8 sum wraps
    for name, kw, want in (("plain", {}, plain),
                           ("relu_x", dict(relu=True, x16=x), np.where(c["x"] > 0, plain, 0).astype(np.int8)),
                           ("relu_pooled", dict(relu=True, pooled=pooled), c["sums_pooled"].astype(np.int8))):
        dx = F.Buf(T, c["x"].shape)
        ops.maxpool_grad_arg(arg, dy, h, w, k, s, p, dx=dx.t, **kw)
        dx.check(want, "dx " + name, bad, tag)


@pytest.mark.parametrize("pool", F.PP_POOLS, ids=_sid)
@pytest.mark.parametrize("geo", PP_GEOS, ids=_sid)
def test_maxpool_grad_arg(T, ops, geo, pool):
    """No relu, relu from x, relu from `pooled`: the generic gather at 2x2 / 2, and at 3x3 / 2 / 1
    the packed kernel for the `pooled` form.  Four windows of 127 wrap to -4."""
    n, h, w, cp = geo
    bad = []
    for relu in (False, True):
        c = F.pp_case(n, h, w, cp, *pool, relu)
        _grad_forms(T, ops, c, h, w, pool, ("G", geo, pool, relu), bad)
    assert not bad, bad


@pytest.mark.parametrize("geo", PP_GEOS, ids=_sid)
def test_maxpool_grad_arg_generic_overlapping(T, ops, geo):
    """A 5x5 / 2 / 2 pool, which only the generic gather takes: the three forms against the
    reference; then niti_maxpool_arg's own positions into the gradient on relu inputs, masked by x,
    against the reference, and on maps of at least 5 x 5 (second assertion) masked by the
    forward's own y, which gives the same."""
    n, h, w, cp = geo
    k, s, p = pool = F.PP_GENERIC_POOL
    bad = []
    for relu in (False, True):
        c = F.pp_case(n, h, w, cp, k, s, p, relu)
        _grad_forms(T, ops, c, h, w, pool, ("G", geo, pool, relu), bad)
    c = F.pp_case(n, h, w, cp, k, s, p, True)
    x = F.dev(T, c["x"])
    y, arg = ops.maxpool_arg(x, k, s, p, ohw=c["y"].shape[1:3])
    dy = F.dev(T, c["dy"])
    by_x = ops.maxpool_grad_arg(arg, dy, h, w, k, s, p, relu=True, x16=x)
    by_y = ops.maxpool_grad_arg(arg, dy, h, w, k, s, p, relu=True, pooled=y)
    want = np.where(c["x"] > 0, c["sums"].astype(np.int8), 0).astype(np.int8)
    assert np.array_equal(by_x.cpu().numpy(), want)
    if min(h, w) >= k:   # whole windows: y is x at each window's first max
        assert np.array_equal(by_y.cpu().numpy(), want) and T.equal(by_x, by_y)
    assert not bad, bad


# --------------------------------------------------------------------------------- host-side rejections
def test_fused_requant_rejections(T, ops):
    """Combinations requant_act cannot run come back INVALID_VALUE before any launch."""
    from niti_amd._lib import NitiError

    def z(*shape, dtype=None):
        return T.zeros(shape, dtype=dtype or T.int8, device="cuda")

    amax = ops.new_range()
    acc = z(64, 48, dtype=T.int32)      # 64 rows of 48 channels
    b = z(64 * 4 * 48)                   # any int8 buffer large enough for every form below
    cases = {
        "odd pool H": dict(out=b, pool_out=b, pool_hw=(3, 4)),
        "dx_c32 with ldc % 32 != 0": dict(pool_x=b, pool_y=b, pool_dx=b, pool_dx_c32=b, pool_hw=(4, 4)),
        "out_p16 with pool_out": dict(out=b, pool_out=b, pool_hw=(4, 4), out_p16=b),
        "pool3 with relu_mask": dict(pool3_out=b, pool3_arg=b, pool3_hw=(8, 8), pool3_ohw=(4, 4), relu_mask=b),
        "pool3 with OH not (H - 1) / 2 + 1": dict(pool3_out=b, pool3_arg=b, pool3_hw=(8, 8), pool3_ohw=(3, 4)),
        "zero_cls with out_p16": dict(out=b, out_p16=b, zero_cls=6, zc_hw=(8, 8)),
        "P16 pool backward with H != W": dict(pool_x=b, pool_y=b, pool_dx=b, out_p16=b, pool_hw=(8, 4)),
    }
    for name, kw in cases.items():
        with pytest.raises(NitiError) as e:
            ops.requant_act_fused(acc, amax, **kw)
        assert e.value.code == 5, name   # INVALID_VALUE
    # rows not a multiple of the P16 pool-backward group: 6 pooled pixels of 2x2 images
    with pytest.raises(NitiError) as e:
        ops.requant_act_fused(acc[:6], amax, pool_x=b, pool_y=b, pool_dx=b, out_p16=b, pool_hw=(2, 2))
    assert e.value.code == 5
    T.cuda.synchronize()
    assert not b.any().item()   # nothing was launched
