#!/usr/bin/env python3
"""The global pool's kernel and a MobileNetV2-shaped chain's step, measured (GPU box; not a test, not part
of bench.py):  python3 tools/skip_bench.py [--reps 50] [--out profiles/sum_pool_wide_bench.txt]

Per shape (n images of hw pixels and cp channels, NHWC16):
  wide   niti_sum_pool_wide, the sums and their range
  old    niti_sum_pool on the same input (one thread per image and channel)
  copy   a device-to-device copy of the input's n * hw * cp bytes (hipMemcpyAsync, called through ctypes as
         the two kernels are), the yardstick of one read of it
Then the README's MobileNetV2-shaped layer list at 32 px and batch 64: ms per training step after autotune
(int8 inputs, direct launches), and the launches the two new rules add, timed alone on the list's own
shapes -- every residual sum's two launches forward and backward (niti_residual_add with z = NULL,
niti_residual_requant) and the global pool's (niti_sum_pool_wide, niti_requant_act, niti_sum_pool_grad) --
as a share of the step.
Times are HIP events around `reps` back-to-back runs on one stream, after 3 warm-up runs, the best of 3.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mandheling-dsp-training_amd"))

import torch  # noqa: E402

from niti_amd import ops  # noqa: E402
from niti_amd.model import NitiModel  # noqa: E402

SHAPES = [(128, 49, 512), (256, 16, 1280), (256, 64, 256), (256, 1024, 64)]  # (n, hw, cp)


def timed(fn, reps):
    st = torch.cuda.current_stream()
    for _ in range(3):
        fn()
    best = 1e30
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        for _ in range(reps):
            fn()
        b.record(st)
        b.synchronize()
        best = min(best, a.elapsed_time(b) / reps * 1e3)
    return best  # us


def mobilenetv2_spec(classes=10):
    """The README's list: a 3x3 stem, the first block without expansion, thirteen inverted-residual blocks
    (expansion 6; the sum where stride and channels keep the shape), 1x1 to 1280, the global pool, fc."""
    def inverted(c_in, c_out, stride, t=6):
        return [dict(c_out=t * c_in, kernel=1, relu=1), dict(kernel=3, pad=1, relu=1, depthwise=1, stride=stride),
                dict(c_out=c_out, kernel=1, skip=3 if stride == 1 and c_in == c_out else 0)]

    cfg = [(16, 24, 1), (24, 24, 1), (24, 32, 2), (32, 32, 1), (32, 32, 1), (32, 64, 2), (64, 64, 1), (64, 64, 1),
           (64, 96, 1), (96, 96, 1), (96, 160, 2), (160, 160, 1), (160, 320, 1)]
    spec = [dict(c_out=32, kernel=3, pad=1, relu=1), dict(kernel=3, pad=1, relu=1, depthwise=1), dict(c_out=16, kernel=1)]
    for c_in, c_out, stride in cfg:
        spec += inverted(c_in, c_out, stride)
    return spec + [dict(c_out=1280, kernel=1, relu=1, gpool=1), (classes, 1)]


def bench_pool(reps, say):
    import ctypes as C

    import niti_amd._lib as L
    lib = L.lib()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    hip = C.CDLL("libamdhip64.so")  # (the runtime torch has loaded)
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    D2D = 3  # hipMemcpyDeviceToDevice
    say("sum_pool_wide against sum_pool and a copy of the input bytes (us; x: old / wide, of copy: wide / copy)")
    say("(all three through ctypes on preallocated buffers, so a figure is the launch and not a Python wrapper)")
    say(f"{'n':>5} {'hw':>5} {'cp':>5} {'wide':>9} {'old':>9} {'copy':>9} {'x':>7} {'of copy':>8}")
    for n, hw, cp in SHAPES:
        x = torch.randint(-128, 128, (n, hw, 1, cp), dtype=torch.int8, device="cuda")
        y = torch.empty_like(x)
        amax = ops.new_range()
        a = ops.sum_pool_wide(x, amax)
        b = ops.sum_pool(x, ops.new_range())
        assert torch.equal(a, b)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        px, py, pa, pb, pm = P(x), P(y), P(a), P(b), P(amax)
        assert hip.hipMemcpyAsync(py, px, x.numel(), D2D, st) == 0
        tw = timed(lambda: lib.niti_sum_pool_wide(px, n, hw, cp, pa, pm, st), reps)
        to = timed(lambda: lib.niti_sum_pool(px, n, hw, cp, pb, pm, st), reps)
        tc = timed(lambda: hip.hipMemcpyAsync(py, px, x.numel(), D2D, st), reps)
        say(f"{n:>5} {hw:>5} {cp:>5} {tw:>9.2f} {to:>9.2f} {tc:>9.2f} {to / tw:>7.2f} {tw / tc:>8.2f}")


def bench_step(reps, say):
    batch, hw = 64, 32
    spec = mobilenetv2_spec()
    m = NitiModel.from_chain(spec, 3, hw, batch)
    m.init_weights(1)
    x = torch.randint(-127, 128, (batch, 3, hw, hw), dtype=torch.int8, device="cuda")
    labels = torch.randint(0, 10, (batch,), dtype=torch.int32, device="cuda")
    m.train_step(x, -3, labels)
    m.autotune(reps=3)
    m.init_weights(1)
    step = timed(lambda: m.train_step(x, -3, labels), max(5, reps // 5))
    # the new rules' launches alone, on the list's shapes: the C entry points on preallocated buffers (the
    # range words are not zeroed between runs: the same data gives the same maximum)
    import ctypes as C

    import niti_amd._lib as L
    lib = L.lib()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e = torch.zeros(1, dtype=torch.int8, device="cuda")
    eo = torch.zeros(1, dtype=torch.int8, device="cuda")
    adds = pool = 0.0
    n_adds = 0
    for l in m.layers:
        cp = (l["c_out"] + 15) // 16 * 16
        if l.get("skip"):
            n_adds += 1
            a = torch.randint(-127, 128, (batch, l["oh"], l["ow"], cp), dtype=torch.int8, device="cuda")
            b = torch.randint(-127, 128, a.shape, dtype=torch.int8, device="cuda")
            out = torch.empty_like(a)
            amax = ops.new_range()
            pa, pb, po, pm, pe, peo, cnt = P(a), P(b), P(out), P(amax), P(e), P(eo), a.numel()

            def fwd():
                lib.niti_residual_add(pa, pe, pb, pe, cnt, None, None, pm, st)
                lib.niti_residual_requant(pa, pe, pb, pe, cnt, pm, None, peo, 0, po, st)

            def bwd():  # (masked, as at a source with a relu)
                lib.niti_residual_add(pa, pe, pb, pe, cnt, None, None, pm, st)
                lib.niti_residual_requant_relu_grad(pa, pe, pb, pe, cnt, pm, None, peo, pb, po, st)

            adds += timed(fwd, reps) + timed(bwd, reps)
        if l.get("gpool"):
            hw_l = l["oh"] * l["ow"]
            a = torch.randint(0, 128, (batch, l["oh"], l["ow"], cp), dtype=torch.int8, device="cuda")
            amax = ops.new_range()
            acc = ops.sum_pool_wide(a, amax)
            g = ops.requant_act(acc, amax)
            dx = torch.empty_like(a)
            pa, pc, pg, pd, pm = P(a), P(acc), P(g), P(dx), P(amax)

            def pool_fwd():
                lib.niti_sum_pool_wide(pa, batch, hw_l, cp, pc, pm, st)
                lib.niti_requant_act(pc, batch, cp, pm, None, None, None, 0, None, pg, st)

            pool += timed(pool_fwd, reps) + timed(lambda: lib.niti_sum_pool_grad(pg, batch, hw_l, cp, pd, st), reps)
    say("")
    say(f"MobileNetV2-shaped list ({len(spec)} layers, {n_adds} sums, 1 global pool), {hw} px, batch {batch}, after autotune:")
    say(f"  step {step / 1e3:.3f} ms")
    say(f"  the sums' launches alone (forward + backward) {adds:.1f} us = {100 * adds / step:.1f} % of the step")
    say(f"  the global pool's launches alone (forward + backward) {pool:.1f} us = {100 * pool / step:.1f} % of the step")
    NitiModel.reset_plans()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/skip_bench.py --reps {args.reps} on {torch.cuda.get_device_name(0)}")
    bench_pool(args.reps, say)
    if not args.no_step:
        bench_step(args.reps, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
