"""The kernels around the GEMMs against the CPU oracle, bit for bit, through the split device API
(niti_amd.ops over the C ABI): the NITI_SGD update with its weight copies, the residual add and its
fused requantisation, niti_requant_act from the op level, the layout helpers and the sum pool.

Cases, references and what each case guards: tests/update_op_cases.py (its tables are checked on
the CPU by tests/test_update_op_cases.py).  Every comparison is np.array_equal against the oracle
or numpy; the only GPU-vs-GPU assertion is the named second one, wf == ops.weights_to_wf."""
import os
import subprocess
import sys

import numpy as np
import pytest

import update_op_cases as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def dev(T, a):
    return T.from_numpy(np.array(a)).cuda()   # (a copy: the cached cases are read-only)


def i8s(T, v):
    return T.tensor([v], dtype=T.int8, device="cuda")


def _lid(layer):
    return "x".join(map(str, layer[:3]))


# ------------------------------------------------------------------------------------ A. SGD update
def _sgd_check(T, ops, layer, rule, pin=None):
    co, ci, kk, with_wf = layer
    acc, w0 = U.sgd_inputs(co, ci, kk, pin)
    ref = U.sgd_reference(co, ci, kk, rule, with_wf, pin)
    k, cip, cop = acc.shape[1], acc.shape[3], U.r16(co)
    d_acc, w16 = dev(T, acc), dev(T, w0)
    amax = ops.new_range()
    ops.absmax(d_acc, amax)
    assert ops.range_max(amax) == int(np.abs(acc.astype(np.int64)).max())
    fill = lambda *shape: T.full(shape, U.SGD_FILL, dtype=T.int8, device="cuda")  # noqa: E731
    wT, g = fill(ci, k, k, cop), fill(co, k, k, cip)
    wf = fill(U.wf_bytes(co, ci)) if with_wf else None
    wft = fill(U.wf_bytes(co, ci)) if with_wf else None
    ops.sgd_update(d_acc, amax, w16, ci, rule, wT=wT, g=g, wf=wf, wft=wft)
    T.cuda.synchronize()
    assert np.array_equal(g.cpu().numpy(), ref["g"])
    w_new = w16.cpu().numpy()
    assert np.array_equal(w_new, ref["w"])
    assert not w_new[..., ci:].any()
    wTn = wT.cpu().numpy()
    assert np.array_equal(wTn[..., :co], ref["w"][..., :ci].transpose(3, 1, 2, 0))
    assert not wTn[..., co:].any()
    assert np.array_equal(wTn, ref["wT"])
    if with_wf:
        assert np.array_equal(wf.cpu().numpy(), ref["wf"])
        assert np.array_equal(wft.cpu().numpy(), ref["wft"])
        # second assertion: the same bytes as the stand-alone layout op on the new weights
        assert T.equal(wf, ops.weights_to_wf(w16, ci, transpose=False))
        assert T.equal(wft, ops.weights_to_wf(w16, ci, transpose=True))


@pytest.mark.parametrize("rule", U.SGD_RULES)
@pytest.mark.parametrize("layer", U.SGD_LAYERS, ids=_lid)
def test_sgd_update_random(T, ops, layer, rule):
    """acc in +-2^20, weights over the whole int8 range: g, w16 with its zero pad lanes, wT with its
    zero columns, wf and wft against the oracle, every buffer pre-filled with 77.  896 x 896 x 9
    makes the update's grid-stride loop iterate."""
    assert U.sgd_reference(*layer[:3], rule, layer[3])["clipped"] >= 1
    _sgd_check(T, ops, layer, rule)


@pytest.mark.parametrize("rule", U.SGD_RULES)
@pytest.mark.parametrize("pin", U.SGD_SMALL_MAX)
@pytest.mark.parametrize("layer", U.SGD_SMALL_LAYERS, ids=_lid)
def test_sgd_update_small_range(T, ops, layer, pin, rule):
    """max|acc| pinned to 0, 1 (bw == 0: no gradient), 2, 3, 5 (shifts -2 .. 1) and 2^31 - 1."""
    _sgd_check(T, ops, layer, rule, pin)


def test_sgd_update_wf_rejects_ragged_channels(T, ops):
    from niti_amd._lib import NitiError
    co, ci = 32, 40
    acc = T.zeros((co, 3, 3, U.r16(ci)), dtype=T.int32, device="cuda")
    w16 = T.zeros((co, 3, 3, U.r16(ci)), dtype=T.int8, device="cuda")
    wf = T.zeros(2 * 9 * 1024, dtype=T.int8, device="cuda")
    with pytest.raises(NitiError) as e:
        ops.sgd_update(acc, ops.new_range(), w16, ci, 2, wf=wf, wft=wf.clone())
    assert e.value.code == 2   # NOT_SUPPORT


# ------------------------------------------------------------------------------------ B. residual ops
def _residual_check(T, ops, case, swap, n):
    amp, gap, e_hi = case[:3]
    a, ea, b, eb, _ = U.res_inputs(amp, gap, e_hi, swap, n)
    ref = U.res_reference(amp, gap, e_hi, swap, n)
    da, db = dev(T, a), dev(T, b)
    amax = ops.new_range()
    z, ez = ops.residual_add(da, i8s(T, ea), db, i8s(T, eb), amax)
    assert np.array_equal(z.cpu().numpy(), ref["z"])
    assert int(ez.item()) == ref["ez"]
    assert ops.range_max(amax) == ref["range"]
    amax2 = ops.new_range()
    ops.residual_range(da, i8s(T, ea), db, i8s(T, eb), amax2)
    assert ops.range_max(amax2) == ref["range"]
    bad = U.residual_requant_mismatch(T, ops, case, swap, n)
    assert not bad, bad


@pytest.mark.parametrize("swap", [False, True], ids=["a_hi", "b_hi"])
@pytest.mark.parametrize("case", U.RES_CASES, ids=lambda c: f"amp{c[0]}-gap{c[1]}")
def test_residual_ops(T, ops, case, swap):
    """residual_add (z, ez, range), residual_range, residual_requant with relu off / on and with
    the relu-gradient mask against residual_add + requant of oracle/niti_resnet_ref.py."""
    _residual_check(T, ops, case, swap, U.RES_N)


@pytest.mark.parametrize("swap", [False, True], ids=["a_hi", "b_hi"])
@pytest.mark.parametrize("case", U.RES_BIG_CASES, ids=lambda c: f"amp{c[0]}-gap{c[1]}")
def test_residual_ops_grid_stride(T, ops, case, swap):
    """n = 2048 * 256 * 16 + 16 * 300: the 2048-block loops take a second, ragged pass."""
    _residual_check(T, ops, case, swap, U.RES_N_BIG)


_CHILD = """
import sys
sys.path[:0] = {paths!r}
import torch
import update_op_cases as U
from niti_amd import ops
bad = U.residual_table_mismatch(torch, ops)
torch.cuda.synchronize()
for b in bad:
    print("MISMATCH", b)
print("checked", len(U.RES_CASES) * 2 * len(U.RES_MODES), "mismatches", len(bad))
sys.exit(1 if bad else 0)
"""


def test_residual_requant_32bit_fallback(T):
    """NITI_RES_PK=0 (read once per process, so a fresh child): the n = 4096 table through
    residual_requant's 32-bit loop, relu off / on and with the mask."""
    paths = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"),
             os.path.join(ROOT, "mandheling-dsp-training_amd")]
    env = dict(os.environ, NITI_RES_PK="0")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert f"checked {len(U.RES_CASES) * 6} mismatches 0" in r.stdout


# ------------------------------------------------------------------------------------ C. requant_act
def _requant_check(T, ops, rows, ldc, pin, exp_in, wscale):
    acc, mask = U.rq_inputs(rows, ldc, pin)
    ref = U.rq_reference(rows, ldc, pin)
    d_acc, d_mask = dev(T, acc), dev(T, mask)
    amax = ops.new_range()
    ops.absmax(d_acc, amax)
    assert ops.range_max(amax) == pin
    want_e = int(np.int32(exp_in + wscale + ref["inc"]).astype(np.int8))   # the int8 exponent wraps
    for key, kw in (("out", {}), ("out_relu", dict(relu=True)), ("out_mask", dict(relu_mask=d_mask))):
        e = i8s(T, 99)
        got = ops.requant_act(d_acc, amax, exp_in=i8s(T, exp_in), wscale=i8s(T, wscale), exp_out=e, **kw)
        assert np.array_equal(got.cpu().numpy(), ref[key]), key
        assert int(e.item()) == want_e, key


@pytest.mark.parametrize("name,pin", U.RQ_PINS, ids=[p[0] for p in U.RQ_PINS])
@pytest.mark.parametrize("shape", U.RQ_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_requant_act_op(T, ops, shape, name, pin):
    """niti_requant_act (requant_quad_kernel<RQ_PLAIN>) with relu off / on and with relu_mask, on
    the raw, shift-1 and PSTO branches; 65600 x 128 runs the four-loads outer loop and its tail."""
    assert U.rq_reference(*shape, pin)["branch"] == name
    _requant_check(T, ops, *shape, pin, *U.RQ_EXP)


def test_requant_act_exponent_wraps(T, ops):
    w = U.RQ_WRAP
    _requant_check(T, ops, *w["shape"], w["pin"], w["exp_in"], w["wscale"])


# ------------------------------------------------------------------------------------ D. layouts, sum pool
@pytest.mark.parametrize("shape", U.LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_helpers(T, ops, shape):
    n, c, h, w = shape
    x, x16 = U.layout_inputs(*shape)
    want = U.chwn16_of(x)
    assert not want[c:].any() and not want[..., n:].any()
    got = ops.nchw_to_chwn16(dev(T, x)).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert not got[c:].any() and not got[..., n:].any()
    got = ops.nhwc16_to_chwn16(dev(T, x16)).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert not got[c:].any() and not got[..., n:].any()
    assert np.array_equal(ops.nhwc16_to_nchw(dev(T, x16), c).cpu().numpy(), x)
    # the same tensor read as weights: OHWI16 [co = n][kh][kw][cip] -> OIHW
    assert np.array_equal(ops.ohwi16_to_oihw(dev(T, x16), c).cpu().numpy(), x)


def test_sum_pool_many_blocks(T, ops):
    n, h, w, cp = U.POOL_SHAPE
    rng = np.random.default_rng(41)
    x = rng.integers(-128, 128, U.POOL_SHAPE).astype(np.int8)
    x[n - 1, :, :, cp - 1] = -128   # the largest sum sits in the last block
    want = x.astype(np.int64).sum(axis=(1, 2))
    amax = ops.new_range()
    acc = ops.sum_pool(dev(T, x), amax).cpu().numpy()
    assert acc.dtype == np.int32 and np.array_equal(acc.astype(np.int64), want)
    assert ops.range_max(amax) == int(np.abs(want).max()) == 128 * h * w
    dy = rng.integers(-128, 128, (n, cp)).astype(np.int8)
    dy[0, 0] = -128
    dx = ops.sum_pool_grad(dev(T, dy), h, w).cpu().numpy()
    assert np.array_equal(dx, np.broadcast_to(dy[:, None, None, :], U.POOL_SHAPE))
