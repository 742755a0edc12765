#!/usr/bin/env python3
"""Grouped conv launches against the dense emulation of the same layer (GPU box; not a test, not part of
bench.py):  python3 tools/grouped_bench.py [--reps 1000] [--stride 2] [--out profiles/grouped_bench.txt]
--stride 2 measures the same layers at stride 2 (h -> h / 2 pixels; niti_gconv2_*, the dense emulation on the
strided op-level GEMM launches) into profiles/grouped_stride2_bench.txt.
--narrow measures group widths 4 and 8 (niti_gconv_narrow_*) at ResNeXt-50 32x4d's shapes, each at its own stride,
into profiles/grouped_narrow_bench.txt.

Per shape (C channels in G groups at h x h pixels, 3x3 pad 1, batch 64) and phase:
  grouped  the niti_gconv_* launches: forward / input gradient = pass 0 (range) + pass 1 (requantise);
           weight gradient = the slab launch + the combine (niti_sgd_combine)
  dense    the same layer the only way the library ran it before: the block-diagonal dense weight on the
           op-level GEMM path (conv_*_acc with its range, then requant_act; weight gradient: conv_wgrad_acc with
           its range over the dense tensor, which is not the layer's).  This is not what the chain driver runs for
           a dense 3x3 layer of these sizes (the row kernels, the speculative pair), which store no int32 tensor.
Times are HIP events around `reps` back-to-back runs on one stream (a window of tens of milliseconds) after 20
warm-up runs, the median of 5 such rounds, taken in both orders (grouped then dense, dense then grouped); both
medians are printed.  MFMA rate: the layer's own multiply-adds (n oh ow C cg 9) x 2, counted once -- the second
pass's recompute of the forward and the input gradient is not useful work -- over the grouped time, against the int8
peak bench.py uses (256 CU x 4 SIMD x 2048 op/clk x 2.4 GHz).
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mandheling-dsp-training_amd"))

import torch  # noqa: E402

import niti_amd._lib as L  # noqa: E402
from niti_amd import ops  # noqa: E402

SHAPES = [(64, 256, 16, 32), (64, 512, 8, 16), (64, 128, 2, 32)]  # (batch, C, G, h)
NARROW_SHAPES = [(64, 128, 32, 56, 1), (64, 256, 32, 56, 2)]  # (batch, C, G, h, stride): stage 1 (cg 4), stage 2's first block (cg 8)
PEAK_INT8_TOPS = 256 * 4 * 2048 * 2.4e9 / 1e12


def timed(fn, reps):
    st = torch.cuda.current_stream()
    for _ in range(20):
        fn()
    rounds = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        for _ in range(reps):
            fn()
        b.record(st)
        b.synchronize()
        rounds.append(a.elapsed_time(b) / reps * 1e3)
    return statistics.median(rounds)  # us


def ok(code):
    assert code == 0, code


def bench_shape(n, c, groups, h, reps, stride=1):
    lib = L.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = ops.geom(n, c, h, h, c, 3, stride=stride, pad=1)
    oh = g.oh
    cg = c // groups
    pre = "gconv_narrow" if cg < 16 else "gconv2" if stride == 2 else "gconv"
    fns = [getattr(lib, f"niti_{pre}_{k}") for k in ("fwd", "dgrad", "wgrad", "wgrad_slabs")]
    dev = "cuda"
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    x = torch.randint(-127, 128, (n, h, h, c), dtype=torch.int8, device=dev)
    dy = torch.randint(-127, 128, (n, oh, oh, c), dtype=torch.int8, device=dev)
    w = torch.randint(-127, 128, (c, cg, 3, 3), dtype=torch.int8, device=dev)
    w16 = ops.gconv_weight(w)
    out, out_d = torch.empty_like(dy), torch.empty_like(x)  # the forward's output, the input gradient's
    amax = ops.new_range()
    o = L.DwconvOut()
    o.out = out.data_ptr()
    o.relu = 1
    o2 = L.DwconvOut()
    o2.out = out_d.data_ptr()

    def g_act(fn, a, oo):
        def run():
            amax.zero_()
            ok(fn(C.byref(g), groups, P(a), P(w16), P(amax), C.byref(oo), 0, s))
            ok(fn(C.byref(g), groups, P(a), P(w16), P(amax), C.byref(oo), 1, s))
        return run

    slabs = int(fns[3](C.byref(g), groups))
    one = c * 9 * max(cg, 16)  # (a width of 4 or 8 pads to 16)
    slab = torch.empty((slabs, one), dtype=torch.int32, device=dev)
    gacc = torch.empty(one, dtype=torch.int32, device=dev)
    job = (L.SgdCombineJob * 1)()
    job[0].slab, job[0].splits, job[0].stride, job[0].n = slab.data_ptr(), slabs, one, one
    job[0].acc, job[0].amax = gacc.data_ptr(), amax.data_ptr()

    def g_wgrad():
        amax.zero_()
        ok(fns[2](C.byref(g), groups, P(x), P(dy), P(slab), slab.numel() * 4, None, s))
        ok(lib.niti_sgd_combine(job, 1, s))

    # the dense emulation: the block-diagonal weight on the op-level GEMM path
    wd = torch.zeros((c, c, 3, 3), dtype=torch.int8, device=dev)
    for k in range(groups):
        wd[k * cg:(k + 1) * cg, k * cg:(k + 1) * cg] = w[k * cg:(k + 1) * cg]
    wd16 = ops.oihw_to_ohwi16(wd)
    wdT = ops.ohwi16_to_ihwo16(wd16, c)
    px, px_o = n * h * h, n * oh * oh
    acc = torch.empty((px, c), dtype=torch.int32, device=dev)
    wacc = torch.empty((c, 3, 3, c), dtype=torch.int32, device=dev)
    wss = [ops.conv_workspace(g, op) for op in (0, 1, 2)]

    def dense_fwd():
        amax.zero_()
        ok(lib.niti_conv_fwd_acc(C.byref(g), P(x), P(wd16), P(acc), P(amax), P(wss[0][0]), wss[0][1], s))
        ok(lib.niti_requant_act(P(acc), px_o, c, P(amax), None, None, None, 1, None, P(out), s))

    def dense_dgrad():
        amax.zero_()
        ok(lib.niti_conv_dgrad_acc(C.byref(g), P(dy), P(wdT), P(acc), P(amax), P(wss[1][0]), wss[1][1], s))
        ok(lib.niti_requant_act(P(acc), px, c, P(amax), None, None, None, 0, None, P(out_d), s))

    def dense_wgrad():
        amax.zero_()
        ok(lib.niti_conv_wgrad_acc(C.byref(g), P(x), P(dy), P(wacc), P(amax), P(wss[2][0]), wss[2][1], s))

    macs = n * oh * oh * c * cg * 9
    rows = {}
    for ph, gf, df in (("fwd", g_act(fns[0], x, o), dense_fwd),
                       ("dgrad", g_act(fns[1], dy, o2), dense_dgrad), ("wgrad", g_wgrad, dense_wgrad)):
        g1, d1 = timed(gf, reps), timed(df, reps)  # grouped first
        d2, g2 = timed(df, reps), timed(gf, reps)  # dense first
        rows[ph] = (g1, d1, g2, d2, 2 * macs / (min(g1, g2) * 1e-6) / 1e12)
    return slabs, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--stride", type=int, default=1, choices=(1, 2))
    ap.add_argument("--narrow", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "grouped_narrow_bench.txt" if args.narrow else
                                        "grouped_stride2_bench.txt" if args.stride == 2 else "grouped_bench.txt")
    shapes = NARROW_SHAPES if args.narrow else [sh + (args.stride,) for sh in SHAPES]
    lines = [f"# tools/grouped_bench.py --reps {args.reps} " + ("--narrow" if args.narrow else f"--stride {args.stride}") +
             f": {torch.cuda.get_device_name(0)}",
             f"# us per phase, medians of 5 rounds of {args.reps} runs: grouped / dense measured grouped-first (1) and",
             "# dense-first (2); dense = the block-diagonal weight on the op-level GEMM path (int32 stored, then requantised);",
             "# dense/grp = the ratio of the two orders' means (above 1: the grouped launches are faster); TOPS = the layer's own",
             f"# int8 operations, counted once (no recompute), over the faster grouped time, peak {PEAK_INT8_TOPS:.0f}",
             f"{'shape':>20} {'phase':>6} {'grp1':>9} {'dense1':>9} {'grp2':>9} {'dense2':>9} {'dense/grp':>10} {'TOPS':>8} {'of peak':>8}"]
    for n, c, groups, h, stride in shapes:
        slabs, rows = bench_shape(n, c, groups, h, args.reps, stride)
        for ph, (g1, d1, g2, d2, tops) in rows.items():
            ratio = (d1 + d2) / (g1 + g2)
            lines.append(f"{f'{c}/G{groups}@{h}px' + ('/2' if stride == 2 else '') + f' b{n}':>20} {ph:>6} {g1:9.2f} {d1:9.2f} {g2:9.2f} {d2:9.2f} {ratio:10.2f} {tops:8.1f} "
                         f"{tops / PEAK_INT8_TOPS:8.4f}" + (f"   ({slabs} slabs)" if ph == "wgrad" else "") +
                         ("   SLOWER than the dense emulation" if ratio < 1 else ""))
        print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
