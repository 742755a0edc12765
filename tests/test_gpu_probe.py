"""The kernel probe and the single-phase entry points of the niti_model_* C ABI (set_probe,
probe_read, probe_pause, probe_read_span, run_phase) on both step drivers: the chain driver (VGG-11,
batch 8) and ResNet-18 (batch 2, 32 px, 10 classes).

The expected launch counts were recorded from the library before the two drivers got their common
base (StepDriver); they pin what each probe point brackets, not a timing.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID_VALUE = 5
LAYER = 1      # VGG-11: conv 64 -> 128 at 16 px; ResNet-18: block 0's conv a
MAX_LAUNCHES = 4

# probe_read()'s count after two training steps with set_probe(LAYER, phase, MAX_LAUNCHES):
#   phase 0: one begin / end pair around the layer's whole forward per step (both drivers: the
#            register-fed row kernel's single fused launch)
#   phase 2: one pair per step around the weight-gradient GEMM launch (the chain driver: the P16
#            kernel's own begin / end events, its split-K reduce excluded; ResNet: the whole
#            conv_wgrad_acc phase)
PROBE_COUNT = {("vgg11", 0): 2, ("vgg11", 2): 2, ("resnet18", 0): 2, ("resnet18", 2): 2}
# probe_read_span()'s count for the same phase-2 case: the in-kernel span slots the P16 weight-gradient
# launches filled, one per step (the chain driver only; ResNet has no span probe)
SPAN_COUNT = {"vgg11": 2, "resnet18": 0}


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def _build(T, arch):
    import niti_amd
    from niti_amd.model import NitiModel
    rng = np.random.default_rng(41)
    if arch == "vgg11":
        import niti_model_ref as R
        W, S = R.init_weights(R.vgg11_layers(), seed=41)
        m = NitiModel(niti_amd.ARCH_VGG11, 8)
        x = rng.integers(-127, 128, (8, 3, 32, 32)).astype(np.int8)
    else:
        import niti_resnet_ref as RR
        W, S = RR.init_weights(RR.resnet18_convs(32, 10), seed=41)
        m = NitiModel(niti_amd.ARCH_RESNET18, 2, 32, 10)
        x = rng.integers(-127, 128, (2, 3, 32, 32)).astype(np.int8)
    for i, (w, s) in enumerate(zip(W, S)):
        m.set_weight(i, w, s)
    labels = rng.integers(0, 10, x.shape[0]).astype(np.int32)
    return m, _dev(T, x), _dev(T, labels)


def _code(fn, *a):
    from niti_amd._lib import NitiError
    with pytest.raises(NitiError) as err:
        fn(*a)
    return err.value.code


@pytest.mark.parametrize("arch", ["vgg11", "resnet18"])
def test_probe_and_run_phase(T, arch):
    m, x, labels = _build(T, arch)
    step = lambda: m.train_step(x, -3, labels)  # noqa: E731
    for phase in (0, 2):
        m.set_probe(LAYER, phase, MAX_LAUNCHES)
        step()
        step()
        ms, count = m.probe_read()
        print("probe", arch, phase, ms, count)
        assert ms > 0 and count == PROBE_COUNT[arch, phase], (phase, ms, count)
        assert m.probe_read()[1] == 0  # reading re-arms from zero
        m.probe_pause(True)
        step()
        assert m.probe_read()[1] == 0
        m.probe_pause(False)
        if phase == 2:
            span_ms, spans = m.probe_read_span()
            print("span", arch, span_ms, spans)
            assert spans == SPAN_COUNT[arch]
            assert (span_ms > 0) == (spans > 0)
            assert m.probe_read_span() == (0, 0)
    assert _code(m.set_probe, LAYER, 0, -1) == INVALID_VALUE
    m.set_probe(-1, 0, 0)  # disarms
    step()
    assert m.probe_read() == (0, 0)
    assert m.probe_read_span() == (0, 0)

    # one layer phase of the last step again: no update, nothing downstream rewritten.  After a
    # training step the layer's forward output predates the step's own NITI_SGD update, so phase 0
    # (which runs on the updated weights) is compared after a forward-only step, whose output and
    # weights belong together; phases 1 and 2 leave the output alone after either kind of step.
    nl = len(m.layers)

    def unchanged_by_phases(phases):
        before = [m.get_weight(i) for i in range(nl)], m.logits(), m.tap(LAYER, 0)
        for p in phases:
            m.run_phase(LAYER, p)
            after = [m.get_weight(i) for i in range(nl)], m.logits(), m.tap(LAYER, 0)
            assert all(np.array_equal(a, b) for a, b in zip(after[0], before[0])), p
            assert after[1][1] == before[1][1] and np.array_equal(after[1][0], before[1][0]), p
            assert np.array_equal(after[2], before[2]), p

    unchanged_by_phases((1, 2))
    m.run_phase(LAYER, 0)
    m.eval_step(x, -3, labels)
    unchanged_by_phases((0, 1, 2))
    # phase 1 where there is no input gradient (the chain's layer 0; ResNet's stem has no dx)
    assert _code(m.run_phase, 0, 1) == INVALID_VALUE
    for layer, p in ((LAYER, 3), (LAYER, -1), (nl, 0), (-1, 0)):
        assert _code(m.run_phase, layer, p) == INVALID_VALUE, (layer, p)
    assert m.rowconv_error() == 0
