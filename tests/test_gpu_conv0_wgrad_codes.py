"""GPU parity of the first layer's weight gradient from the pooled gradient and the pool codes
(conv0_wgrad_codes_kernel through niti_conv0_wgrad_codes) and of the training step that takes it,
against the CPU oracle, bit for bit (tests/conv0_wgrad_codes_cases.py holds inputs and references).

Op level: batches 1, 3, 5, 16 x four geometries x three channel pairs, each on the default grid, on
one workgroup (every step on four waves, one slab) and on three.  The codes are the ones conv0_fwd
records where it takes the geometry (32-pixel rows, c_out a multiple of 32 after rounding to 16: the
(64, 64) and (20, 32) pairs at 32x32), compared there against the oracle's route; elsewhere the codes
are derived from the oracle's forward (first_layer_cases.pool_code_of).

Model level, keep_grads(0), two steps against the oracle: VGG-11 at batches 4 and 36 with the route
forced on and off, a chain whose first layer is 8 pixels wide (the route does not apply: its forward
records no codes) and one at 32 pixels with a 32-channel first layer, and the configurations that keep
the old launches: keep_grads(1), two in-process ranks, a captured step, the side stream.
"""
import functools

import numpy as np
import pytest

import chain_cases as CC
import conv0_wgrad_codes_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu_codes(T, case, batch, co, cop):
    """conv0_fwd's recorded route for the case's input (relu, 2x2 pool), [n*ph*pw][cop]."""
    from niti_amd import ops
    import first_layer_cases as F
    g = ops.geom(batch, 32, case["oh"], case["ow"], co, 1)
    assert g.cop == cop
    xcol, wd = _dev(T, case["xcol"]), _dev(T, F.wcol_of(case["w"], cop))
    amax = ops.new_range()
    ops.conv0_fwd(g, xcol, wd, amax, 0)
    px = batch * (case["oh"] // 2) * (case["ow"] // 2)
    pool = T.full((px, cop), 77, dtype=T.int8, device="cuda")
    code = T.full((px, cop), 77, dtype=T.int8, device="cuda")
    ops.conv0_fwd(g, xcol, wd, amax, 1, pool_out=pool, pool_code=code, relu=True)
    return code


def _run_op(T, case, batch, pair, code=None):
    from niti_amd import ops
    co, cop = pair
    g = ops.geom(batch, 32, case["oh"], case["ow"], co, 1)
    xcol, g0 = _dev(T, case["xcol"]), _dev(T, case["g0"])
    code = _dev(T, case["code"]) if code is None else code
    ref = case["ref"]
    want_max = int(np.abs(ref.astype(np.int64)).max())
    steps = -(-batch * (case["oh"] // 2) * (case["ow"] // 2) // 64)
    for blocks in K.BLOCKS:
        acc, rng = ops.conv0_wgrad_codes(g, g0, code, xcol, blocks=blocks, k=case["k"], cop=cop)
        assert np.array_equal(acc.cpu().numpy(), ref), (blocks, steps)
        assert rng == want_max, (blocks, steps)


@pytest.mark.parametrize("pair", K.PAIRS)
@pytest.mark.parametrize("geom", K.GEOMS)
@pytest.mark.parametrize("batch", K.BATCHES)
def test_op_vs_oracle(T, batch, geom, pair):
    case = K.op_case(batch, geom, pair)
    co, cop = pair
    code = None
    if case["ow"] % 32 == 0 and (co + 15) // 16 * 16 == cop:
        # the codes the forward records; once per geometry against the oracle's route (real channels)
        code = _gpu_codes(T, case, batch, co, cop)
        assert np.array_equal(code.cpu().numpy()[:, :co], case["code"][:, :co])
    _run_op(T, case, batch, pair, code)


@pytest.mark.parametrize("kind", K.KINDS[1:])
@pytest.mark.parametrize("geom", [K.GEOMS[2], K.GEOMS[3]])
def test_op_route_edges(T, geom, kind):
    """A zero gradient; every pooled value <= 0 under relu (all codes zero, a zero result); every
    window routed to one element t, and the tie that goes to the first; operands at +-127.  Batch 3,
    at 32x32 with conv0_fwd's own codes and at LeNet's geometry with the oracle's."""
    batch, pair = 3, (64, 64)
    case = K.op_case(batch, geom, pair, kind)
    co, cop = pair
    if kind == "dead_relu":
        assert not case["code"].any() and not case["ref"].any()
    if kind == "zero_grad":
        assert not case["ref"].any()
    if kind.startswith("route") or kind == "tie":
        t = 0 if kind == "tie" else int(kind[-1])
        assert (case["code"][:, :co] == (1 << t)).all()
    code = None
    if case["ow"] % 32 == 0:
        code = _gpu_codes(T, case, batch, co, cop)
        assert np.array_equal(code.cpu().numpy()[:, :co], case["code"][:, :co])
    _run_op(T, case, batch, pair, code)


def test_op_refusals(T):
    """Odd oh, cop = 48 and more than 32 columns: NITI_INVALID_VALUE and an untouched slab."""
    import ctypes as C

    from niti_amd import _lib as L
    lib = L.lib()
    n = 2
    g0 = T.zeros((n * 16 * 16, 64), dtype=T.int8, device="cuda")
    xcol = T.zeros((n * 32 * 32, 32), dtype=T.int8, device="cuda")
    slab = T.full((256, 64 * 32), 7, dtype=T.int32, device="cuda")
    wrote = C.c_int(-1)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for oh, ow, cop, k in ((31, 32, 64, 27), (32, 31, 64, 27), (32, 32, 48, 27), (32, 32, 64, 33)):
        rc = lib.niti_conv0_wgrad_codes(n, oh, ow, cop, k, p(g0), p(g0), p(xcol), 0, p(slab), slab.numel() * 4,
                                        C.byref(wrote), None)
        assert rc == L.INVALID_VALUE, (oh, ow, cop, k)
        assert lib.niti_conv0_wgrad_codes_slabs(n, oh, ow, cop, k, 0) == 0
    T.cuda.synchronize()
    assert wrote.value == -1 and bool((slab == 7).all())


# ---------------------------------------------------------------------------------------- models
def _mode(mode, blocks=0):
    from niti_amd import _lib as L
    L.lib().niti_diag_conv0_wgrad_codes(mode)
    L.lib().niti_diag_conv0_wgrad_blocks(blocks)


def _launches():
    from niti_amd import _lib as L
    return int(L.lib().niti_diag_conv0_wgrad_codes_launches())


def _vgg11(T, batch, mode, *, blocks=0, keep=False, graph=False, overlap=False):
    """Two VGG-11 steps under niti_diag_conv0_wgrad_codes(mode): per step (logits, exponent, sha256 of
    every layer's weights), and the new kernel's launch count."""
    import niti_amd
    from niti_amd.model import NitiModel
    W, S = K.vgg11_weights()
    _mode(mode, blocks)
    try:
        m = NitiModel(niti_amd.ARCH_VGG11, batch)
        m.set_graph(graph)
        m.set_overlap(overlap)
        m.keep_grads(keep)
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
        n0 = _launches()
        out = []
        for x, labels in K.vgg11_data(batch):
            m.train_step(_dev(T, x), -3, _dev(T, labels))
            logits, e = m.logits()
            out.append(dict(logits=logits, exp=e, w=[K.sha(m.get_weight(i)) for i in range(len(W))]))
        assert m.rowconv_error() == 0
        return out, _launches() - n0, m
    finally:
        _mode(-1)


def _same(got, ref, what):
    for step, (a, b) in enumerate(zip(got, ref)):
        assert a["exp"] == b["exp"] and np.array_equal(a["logits"], b["logits"]), (what, "logits", step)
        for i, (x, y) in enumerate(zip(a["w"], b["w"])):
            assert x == y, (what, "weights", step, i)


@pytest.mark.parametrize("batch", [4, 36])
def test_vgg11_on_off_oracle(T, batch):
    """Route forced on (also with three workgroups: several steps a wave) and off: equal to each other
    and to the oracle; the counter moves only when on.  The first layer's dy tap, which a step on
    the route never writes, is rebuilt from the pooled gradient and the codes: equal to the old path's."""
    ref = K.vgg11_ref(batch)
    on, n_on, m = _vgg11(T, batch, 1)
    dy0, dy1 = m.tap(0, 2), m.tap(1, 2)
    on3, n_on3, _ = _vgg11(T, batch, 1, blocks=3)
    off, n_off, m = _vgg11(T, batch, 0)
    assert dy0.any() and np.array_equal(m.tap(0, 2), dy0) and np.array_equal(m.tap(1, 2), dy1)
    assert (n_on, n_on3, n_off) == (K.STEPS, K.STEPS, 0)
    _same(on, ref, "on")
    _same(on3, ref, "on, 3 workgroups")
    _same(off, ref, "off")


@pytest.mark.parametrize("how", ["keep_grads", "graph", "overlap"])
def test_vgg11_old_path_configurations(T, how):
    """keep_grads(1), a captured step and the side stream keep the old launches under mode 1: the
    counter stays 0 and the results are the oracle's."""
    got, n, _ = _vgg11(T, 4, 1, keep=how == "keep_grads", graph=how == "graph", overlap=how == "overlap")
    assert n == 0
    _same(got, K.vgg11_ref(4), how)


def test_vgg11_two_ranks(T):
    """Two in-process ranks of batch 2 (exact mode) under mode 1: no launch of the new kernel, and the
    batch-4 oracle's logits and weights."""
    import ctypes as C

    import niti_amd
    import test_dp_local as TD
    from niti_amd.model import LocalGroup, NitiModel
    W, S = K.vgg11_weights()
    ref = K.vgg11_ref(4)
    world, b = 2, 2
    _mode(1)
    try:
        ranks = [NitiModel(niti_amd.ARCH_VGG11, b) for _ in range(world)]
        group = LocalGroup(world)
        for r, m in enumerate(ranks):
            m.attach_local(group, r, exact=True)
            m.set_overlap(False)
            m.keep_grads(False)
            for i, (w, s) in enumerate(zip(W, S)):
                m.set_weight(i, w, s)
        n0 = _launches()
        streams = [T.cuda.Stream() for _ in range(world)]
        for step, (x, labels) in enumerate(K.vgg11_data(b * world)):
            xd, ld = _dev(T, x), _dev(T, labels)
            parts = [(xd[r * b:(r + 1) * b].contiguous(), ld[r * b:(r + 1) * b].contiguous()) for r in range(world)]
            T.cuda.synchronize()

            def rank_step(r):
                ranks[r].train_step(parts[r][0], -3, parts[r][1], stream=C.c_void_p(streams[r].cuda_stream))
                streams[r].synchronize()

            TD._in_threads([lambda r=r: rank_step(r) for r in range(world)])
            for r, m in enumerate(ranks):
                lg, e = m.logits()
                assert e == ref[step]["exp"] and np.array_equal(lg, ref[step]["logits"][r * b:(r + 1) * b]), (step, r)
                for i in range(len(W)):
                    assert K.sha(m.get_weight(i)) == ref[step]["w"][i], (step, r, i)
        assert _launches() == n0
    finally:
        _mode(-1)


@functools.lru_cache(maxsize=None)
def _chain_ref(net_key, batch):
    import niti_model_ref as R
    net = {"8": K.CHAIN_8, "32": K.CHAIN_32}[net_key]
    layers = CC.derive(net)
    W, S = R.init_weights(layers, seed=29)
    data = CC.batches(layers, batch, K.STEPS, 31)
    return net, layers, W, S, data, CC.ref_steps(layers, W, S, data)


def _chain(T, net_key, batch, mode):
    from niti_amd.model import NitiModel
    net, layers, W, S, data, ref = _chain_ref(net_key, batch)
    in_c, in_hw, spec = net
    _mode(mode)
    try:
        m = NitiModel.from_chain(spec, in_c, in_hw, batch)
        m.set_overlap(False)
        m.keep_grads(False)
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
        n0 = _launches()
        for step, ((x, labels), (newW, rec, _, _)) in enumerate(zip(data, ref)):
            m.train_step(_dev(T, x), -3, _dev(T, labels))
            logits, e = m.logits()
            assert e == rec["exp"][-1] and np.array_equal(logits, rec["logits"]), (mode, step)
            for i in range(len(layers)):
                assert np.array_equal(m.get_weight(i), newW[i]), (mode, step, i)
        assert m.rowconv_error() == 0
        return _launches() - n0
    finally:
        _mode(-1)


def test_chain_8_wide(T):
    """conv 3 -> 32 at 8x8, pool, conv 32 -> 32, pool, head: the oracle's results in both modes; the
    first layer's forward records no codes at 8 pixels, so neither mode launches the new kernel."""
    assert (_chain(T, "8", 6, 1), _chain(T, "8", 6, 0)) == (0, 0)


def test_chain_32_wide_cop32(T):
    """A 20-channel (cop 32) first layer at 32x32 pooled into a row-kernel layer, batch 6 (24 steps):
    the route runs when forced on, and both modes give the oracle's results."""
    assert (_chain(T, "32", 6, 1), _chain(T, "32", 6, 0)) == (K.STEPS, 0)
