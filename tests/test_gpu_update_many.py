"""GPU parity of the job-list update launch (niti_sgd_update_many) against the CPU reference of
tests/update_op_cases.py: three 512 x 512 x 9 jobs of different rule classes in one launch.

Each job has 8 x 8 x 9 = 576 tiles, 1728 in all on the launch's 1536-block grid, so 192 workgroups
take a second tile 1536 further on -- in another job, whose range and rule class differ from the
first one's: an ordinary range (psto_fast), an all-zero gradient (bw == 0: g = 0, w unchanged) and
range 2 under rule 3 (shift -2: psto_generic).
"""
import numpy as np
import pytest

import update_op_cases as U

pytestmark = pytest.mark.gpu

# (pin, rule): update_op_cases.sgd_inputs' pinned range (None: +-2^20)
JOBS = [(None, 2), (0, 2), (2, 3)]
CO = CI = 512


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def test_three_jobs_of_three_rule_classes(T):
    import niti_oracle as O
    from niti_amd import ops
    jobs, refs = [], []
    for pin, rule in JOBS:
        acc, w16 = U.sgd_inputs(CO, CI, 9, pin)
        ref = U.sgd_reference(CO, CI, 9, rule, True, pin)
        bw = O.range_estimate(acc)
        refs.append(ref)
        d_acc = T.from_numpy(np.array(acc)).cuda()
        amax = ops.new_range()
        ops.absmax(d_acc, amax)
        fill = lambda shape: T.full(shape, U.SGD_FILL, dtype=T.int8, device="cuda")  # noqa: E731
        jobs.append(dict(acc=d_acc, amax=amax, w16=T.from_numpy(np.array(w16)).cuda(), ci=CI, rule=rule,
                         wT=fill(ref["wT"].shape), g=fill(ref["g"].shape), wf=fill(ref["wf"].shape),
                         wft=fill(ref["wft"].shape), bw=bw))
    # the classes the three jobs are meant to reach
    assert 0 <= jobs[0]["bw"] - 2 <= 30 and jobs[0]["bw"] > 0
    assert jobs[1]["bw"] == 0
    assert jobs[2]["bw"] - 3 < 0 and jobs[2]["bw"] > 0
    ops.sgd_update_many(jobs)
    for j, (job, ref) in enumerate(zip(jobs, refs)):
        for got, key in (("w16", "w"), ("wT", "wT"), ("g", "g"), ("wf", "wf"), ("wft", "wft")):
            assert np.array_equal(job[got].cpu().numpy(), ref[key]), (j, key)
    assert refs[0]["clipped"] > 0
    assert not refs[1]["g"].any()
