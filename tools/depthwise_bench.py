#!/usr/bin/env python3
"""Depthwise conv launches against two yardsticks measured in the same run (GPU box; not a test, not
part of bench.py):  python3 tools/depthwise_bench.py [--reps 50] [--out profiles/depthwise_bench.txt]
                    python3 tools/depthwise_bench.py --stride 2 --out profiles/depthwise_stride2_bench.txt

Per shape (C channels at h x h pixels, 3x3 pad 1 unless --k 5; --stride 2: MobileNet's downsampling layers,
64 @ 112 -> 56, 128 @ 56 -> 28, 256 @ 28 -> 14, 512 @ 14 -> 7, through niti_dwconv2_*) and phase:
  dw     the depthwise launches: forward / input gradient = pass 0 (range) + pass 1 (requantise);
         weight gradient = the slab launch + the combine (niti_sgd_combine)
  copy   a device-to-device copy that moves the phase's algorithmic bytes: forward / input gradient read
         the input twice and write the output once (3 bytes per element: a copy of 1.5 n bytes); the
         weight gradient reads x and dy once (2 bytes per element: a copy of n bytes).  At stride 2 the
         output is a quarter of the input: forward 2 in + out, input gradient 2 out + in, weight gradient in + out
  dense  the same layer the only way the library ran it before: a block-diagonal dense layer on the
         op-level GEMM path (conv_*_acc with its range, then requant_act; weight gradient: conv_wgrad_acc
         + absmax over the dense tensor, whose range is not the layer's)
Times are HIP events around `reps` back-to-back runs on one stream, after 3 warm-up runs, the best of 3.
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mandheling-dsp-training_amd"))

import torch  # noqa: E402

import niti_amd._lib as L  # noqa: E402
from niti_amd import ops  # noqa: E402

SHAPES = [(256, 64, 32), (256, 128, 16), (256, 256, 8), (256, 512, 4), (32, 64, 112)]  # (batch, C, h)
SHAPES_STRIDE2 = [(32, 64, 112), (32, 128, 56), (32, 256, 28), (32, 512, 14)]


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


def ok(code):
    assert code == 0, code


def bench_shape(n, c, h, k, reps, stride=1):
    lib = L.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pad = k // 2
    g = ops.geom(n, c, h, h, c, k, stride=stride, pad=pad)
    dev = "cuda"
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    fwd_fn, dgrad_fn, wgrad_fn = ((lib.niti_dwconv_fwd, lib.niti_dwconv_dgrad, lib.niti_dwconv_wgrad) if stride == 1 else
                                  (lib.niti_dwconv2_fwd, lib.niti_dwconv2_dgrad, lib.niti_dwconv2_wgrad))
    elems, oelems = n * h * h * g.cip, n * g.oh * g.ow * g.cip
    # the phases' algorithmic bytes (at stride 1: 3 / 3 / 2 per element)
    nbytes = {"fwd": 2 * elems + oelems, "dgrad": 2 * oelems + elems, "wgrad": elems + oelems}
    x = torch.randint(-127, 128, (n, h, h, g.cip), dtype=torch.int8, device=dev)
    dy = torch.randint(-127, 128, (n, g.oh, g.ow, g.cip), dtype=torch.int8, device=dev)
    w = torch.randint(-127, 128, (c, 1, k, k), dtype=torch.int8, device=dev)
    w16 = ops.dwconv_weight(w)
    out = torch.empty_like(x)  # (the larger of the two outputs)
    amax = ops.new_range()
    o = L.DwconvOut()
    o.out = out.data_ptr()
    o.relu = 1

    def dw_act(fn):
        def run():
            amax.zero_()
            ok(fn(C.byref(g), P(x), P(w16), P(amax), C.byref(o), 0, s))
            ok(fn(C.byref(g), P(x), P(w16), P(amax), C.byref(o), 1, s))
        return run

    o2 = L.DwconvOut()
    o2.out = out.data_ptr()
    slabs = ops.dwconv2_wgrad_slabs(g)
    slab = torch.empty((slabs, k * k * g.cip), dtype=torch.int32, device=dev)
    dwacc = torch.empty(k * k * g.cip, dtype=torch.int32, device=dev)
    job = (L.SgdCombineJob * 1)()
    job[0].slab, job[0].splits, job[0].stride, job[0].n = slab.data_ptr(), slabs, k * k * g.cip, k * k * g.cip
    job[0].acc, job[0].amax = dwacc.data_ptr(), amax.data_ptr()

    def dw_wgrad():
        amax.zero_()
        ok(wgrad_fn(C.byref(g), P(x), P(dy), P(slab), slab.numel() * 4, None, s))
        ok(lib.niti_sgd_combine(job, 1, s))

    def dw_dgrad_run():
        amax.zero_()
        ok(dgrad_fn(C.byref(g), P(dy), P(w16), P(amax), C.byref(o2), 0, s))
        ok(dgrad_fn(C.byref(g), P(dy), P(w16), P(amax), C.byref(o2), 1, s))

    src = torch.empty(max(nbytes.values()) // 2, dtype=torch.int8, device=dev)
    dst = torch.empty_like(src)
    copy = lambda ph: timed(lambda: dst[:nbytes[ph] // 2].copy_(src[:nbytes[ph] // 2]), reps)  # noqa: E731
    rows = {}
    rows["fwd"] = [timed(dw_act(fwd_fn), reps), copy("fwd")]
    rows["dgrad"] = [timed(dw_dgrad_run, reps), rows["fwd"][1] if stride == 1 else copy("dgrad")]
    rows["wgrad"] = [timed(dw_wgrad, reps), copy("wgrad")]

    # the dense emulation: W[o][i] = (o == i) ? w[o] : 0 on the op-level GEMM path
    wd = torch.zeros((c, c, k, k), dtype=torch.int8, device=dev)
    idx = torch.arange(c, device=dev)
    wd[idx, idx] = w[:, 0]
    wd16 = ops.oihw_to_ohwi16(wd)
    wdT = ops.ohwi16_to_ihwo16(wd16, c)
    opx = n * g.oh * g.ow
    acc = torch.empty((n * h * h, g.cop), dtype=torch.int32, device=dev)
    wacc = torch.empty((c, k, k, g.cip), dtype=torch.int32, device=dev)
    wss = [ops.conv_workspace(g, op) for op in (0, 1, 2)]

    def dense_fwd():
        amax.zero_()
        ok(lib.niti_conv_fwd_acc(C.byref(g), P(x), P(wd16), P(acc), P(amax), P(wss[0][0]), wss[0][1], s))
        ok(lib.niti_requant_act(P(acc), opx, g.cop, P(amax), None, None, None, 1, None, P(out), s))

    def dense_dgrad():
        amax.zero_()
        ok(lib.niti_conv_dgrad_acc(C.byref(g), P(dy), P(wdT), P(acc), P(amax), P(wss[1][0]), wss[1][1], s))
        ok(lib.niti_requant_act(P(acc), n * h * h, g.cip, P(amax), None, None, None, 0, None, P(out), s))

    def dense_wgrad():
        amax.zero_()
        ok(lib.niti_conv_wgrad_acc(C.byref(g), P(x), P(dy), P(wacc), P(amax), P(wss[2][0]), wss[2][1], s))

    rows["fwd"].append(timed(dense_fwd, reps))
    rows["dgrad"].append(timed(dense_dgrad, reps))
    rows["wgrad"].append(timed(dense_wgrad, reps))
    return nbytes, slabs, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--k", type=int, default=3, choices=[3, 5])
    ap.add_argument("--stride", type=int, default=1, choices=[1, 2])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depthwise_bench.txt"))
    args = ap.parse_args()
    lines = [f"# tools/depthwise_bench.py --reps {args.reps} --k {args.k}" + (" --stride 2" if args.stride == 2 else "") +
             f": {torch.cuda.get_device_name(0)}",
             "# us per phase: dw = the depthwise launches, copy = a copy moving the phase's algorithmic bytes,",
             "# dense = the block-diagonal dense layer on the op-level GEMM path",
             f"{'shape':>18} {'phase':>6} {'MB':>8} {'dw':>9} {'copy':>9} {'dense':>9} {'dw/copy':>8} {'dense/dw':>9} {'GB/s':>8}"]
    for n, c, h in (SHAPES if args.stride == 1 else SHAPES_STRIDE2):
        nbytes, slabs, rows = bench_shape(n, c, h, args.k, args.reps, args.stride)
        for ph, (dw, cp, dn) in rows.items():
            mb = nbytes[ph] / 1e6
            lines.append(f"{f'{c}@{h}px' + ('/2' if args.stride == 2 else '') + f' b{n}':>18} {ph:>6} {mb:8.1f} {dw:9.2f} {cp:9.2f} {dn:9.2f} {dw / cp:8.2f} "
                         f"{dn / dw:9.2f} {mb / dw * 1e3:8.0f}" + (f"   ({slabs} slabs)" if ph == "wgrad" else ""))
        print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
