"""GPU parity of the update launch under the update-bits rule (niti_sgd_update_many_bits) against
the rule restated from the oracle's primitives (tests/update_bits_cases.py), bit for bit.

Every bits value 0..7 is crossed with gradients whose range puts bw - bits below zero, at 0, at 1,
at an odd and at an even shift, and with bw == 0, on the smallest shapes that reach each path of
the update tile: one full 64 x 64 tile, a ragged tile, the fragment-major copies, the transposed
copy over two tiles, a stride-2 layer's sub-pixel class weights, and a deferred split-K combine.
Every output buffer starts as a sentinel: a frozen job (bits == 0) must leave all of them as they
were except the kept gradient, which reads zero.
"""
import numpy as np
import pytest

import update_bits_cases as UB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _job(T, ops, name, bw):
    """(job dict for ops.sgd_update_many*, the device buffers by expected()'s keys)."""
    s = UB.SHAPES[name]
    acc, w = UB.inputs(name, bw)
    a16, w16 = UB.ohwi16(acc), UB.ohwi16(w)
    co, ci, k = s["co"], s["ci"], s["k"]
    dev = lambda v: T.from_numpy(np.array(v)).cuda()  # noqa: E731
    fill = lambda *shape: T.full(shape, UB.FILL, dtype=T.int8, device="cuda")  # noqa: E731
    amax = ops.new_range()
    job = dict(amax=amax, w16=dev(w16), ci=ci, g=fill(*a16.shape))
    if s.get("splits"):
        # the gradient arrives as slabs: acc holds garbage until the launch's combine sums them
        job["slab"] = dev(UB.slabs_of(a16, s["splits"], bw))
        job["acc"] = T.full(a16.shape, 123456, dtype=T.int32, device="cuda")
    else:
        job["acc"] = dev(a16)
        ops.absmax(job["acc"], amax)
    if s.get("wT"):
        job["wT"] = fill(ci, k, k, UB.r16(co))
    if s.get("wf"):
        job["wf"] = fill(UB.U.wf_bytes(co, ci))
        job["wft"] = fill(UB.U.wf_bytes(co, ci))
    if s.get("subw"):
        job["subw"] = fill(ci * k * k * UB.r16(co))
        job["sub"] = (k, k, s["pad"], s["pad"])
    return job, w16


def _check(job, w16, want, tag):
    got = {"w": job["w16"], "g": job["g"], "wT": job.get("wT"), "wf": job.get("wf"), "wft": job.get("wft"),
           "subw": job.get("subw")}
    for key, buf in got.items():
        if buf is None:
            continue
        have = buf.cpu().numpy()
        if want["frozen"] and key != "g":
            ref = w16 if key == "w" else np.full(have.shape, UB.FILL, np.int8)  # untouched
        else:
            ref = want[key]
        assert ref is not None and np.array_equal(have.reshape(ref.shape), ref), (tag, key)


@pytest.mark.parametrize("bits", UB.BITS)
@pytest.mark.parametrize("name", list(UB.SHAPES))
def test_every_bits_value_and_shift_class(T, name, bits):
    from niti_amd import ops
    dbits = T.tensor([bits], dtype=T.int32, device="cuda")
    for shift, bw in UB.classes_of(bits):
        job, w16 = _job(T, ops, name, bw)
        ops.sgd_update_many_bits([job], dbits)
        _check(job, w16, UB.expected(name, bw, bits), (name, bits, shift))
        if UB.SHAPES[name].get("splits"):  # the combine ran whatever the bits: acc is the slabs' sum
            assert np.array_equal(job["acc"].cpu().numpy(), UB.ohwi16(UB.inputs(name, bw)[0]))


def test_three_jobs_of_different_bits_in_one_launch(T):
    from niti_amd import ops
    jobs, keep = [], []
    for name, bits, shift in UB.THREE_JOBS:
        bw = UB.bw_of(bits, shift)
        job, w16 = _job(T, ops, name, bw)
        jobs.append(job)
        keep.append((name, bw, bits, w16))
    dbits = T.tensor([b for _, b, _ in UB.THREE_JOBS], dtype=T.int32, device="cuda")
    ops.sgd_update_many_bits(jobs, dbits)
    for j, (job, (name, bw, bits, w16)) in enumerate(zip(jobs, keep)):
        _check(job, w16, UB.expected(name, bw, bits), ("three", j))


@pytest.mark.parametrize("name", ["tile64", "ragged", "wf", "wT"])
def test_immediate_rule_2_equals_bits_2(T, name):
    """niti_sgd_update_many with rule = 2 and the table word 2 give the same bytes, the reference's
    negative shift at bw == 1 included."""
    from niti_amd import ops
    dbits = T.tensor([2], dtype=T.int32, device="cuda")
    for shift, bw in UB.classes_of(2):
        a, w16 = _job(T, ops, name, bw)
        b, _ = _job(T, ops, name, bw)
        ops.sgd_update_many([dict(a, rule=2)])
        ops.sgd_update_many_bits([b], dbits)
        for key in ("w16", "g", "wT", "wf", "wft"):
            if key in a:
                assert np.array_equal(a[key].cpu().numpy(), b[key].cpu().numpy()), (name, shift, key)
        _check(a, w16, UB.expected(name, bw, 2), (name, "rule2", shift))


def test_refusals(T):
    from niti_amd import ops
    from niti_amd._lib import NitiError
    job, _ = _job(T, ops, "wf", 5)
    dbits = T.tensor([3], dtype=T.int32, device="cuda")
    bad = dict(job, ci=24)  # fragment-major copies need ci % 32 == 0
    with pytest.raises(NitiError):
        ops.sgd_update_many_bits([bad], dbits)
    with pytest.raises(NitiError):
        ops.sgd_update_many_bits([job] * 25, T.full((25,), 3, dtype=T.int32, device="cuda"))
    with pytest.raises(NitiError):  # the immediate entry points keep their rule 2 / 3 validation
        ops.sgd_update_many([dict(job, rule=5)])
    assert np.array_equal(job["g"].cpu().numpy(), np.full(tuple(job["g"].shape), UB.FILL, np.int8))
