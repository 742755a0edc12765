#!/usr/bin/env python3
"""Measurements of the device-resident dataset path ("Device-resident dataset").

  gather   niti_batch_gather alone, HIP events around back-to-back launches, at 256x3x32x32,
           128x3x224x224 and 64x1x28x28: the plain path (no xform), the transformed path (random
           crop offsets in [-4, 4] and flips) and a device-to-device copy of the same bytes (the
           reference point), with the two ratios over the copy.
  loop     VGG-11 at batch 256, one model: `--loop-steps` dataset steps enqueued as fit_epoch does
           (one train_steps call, no synchronisation inside) against as many train_step_images
           calls on one resident batch, alternating, `--rounds` times each; ms per step and the
           difference.
  eval     evaluation throughput through evaluate_dataset against evaluate on the same images
           already on the device.

  resize   the crop-and-resize gather (orders with windows) at 128x3x224x224 from 256x256 stored
           images, with random-resized-crop windows and with centre 224 windows, and at 256x3x32x32
           from 40x40 stored images: against the transformed gather at the same output shape and
           against a device-to-device copy that moves the bytes it must touch (the windows' bytes
           read plus the output bytes written: a copy of half their sum, which reads and writes
           that many).  Then ResNet-18 at batch 128 and 224 px: the dataset loop with
           random-resized-crop from 256x256 stored images against steps on one resident batch.

Needs a GPU; prints one JSON object per section and a closing summary line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mandheling-dsp-training_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def event_ms(torch, fn, reps, windows=5):
    """median and min over `windows` event-bracketed runs of `reps` back-to-back calls, in ms per call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return statistics.median(out), min(out)


def bench_gather(torch, reps):
    from niti_amd import DeviceDataset, make_order
    rows = []
    for n, c, h, w in ((256, 3, 32, 32), (128, 3, 224, 224), (64, 1, 28, 28)):
        count = 4 * n
        g = torch.Generator(device="cuda").manual_seed(n)
        data = torch.randint(0, 256, (count, c, h, w), dtype=torch.uint8, device="cuda", generator=g)
        labels = torch.randint(0, 10, (count,), dtype=torch.int32, device="cuda", generator=g)
        ds = DeviceDataset(data, labels)
        index, xform = make_order(count, n, seed=1, epoch=0, pad=4, flip=True)
        out = torch.empty((n, c, h, w), dtype=torch.uint8, device="cuda")
        lab = torch.empty(n, dtype=torch.int32, device="cuda")
        src = data[:n]
        nbytes = n * c * h * w
        steps = len(index) // n
        k = [0]

        def gather():
            ds.gather((k[0] % steps) * n, n, out, lab)
            k[0] += 1

        ds.set_order(index, None)
        plain = event_ms(torch, gather, reps)
        ds.set_order(index, xform)
        xf = event_ms(torch, gather, reps)
        copy = event_ms(torch, lambda: out.copy_(src), reps)
        row = {"section": "gather", "shape": f"{n}x{c}x{h}x{w}", "bytes": nbytes, "launches_per_window": reps,
               "plain_us": round(plain[0] * 1e3, 2), "xform_us": round(xf[0] * 1e3, 2), "copy_us": round(copy[0] * 1e3, 2),
               "plain_us_min": round(plain[1] * 1e3, 2), "xform_us_min": round(xf[1] * 1e3, 2),
               "copy_us_min": round(copy[1] * 1e3, 2),
               "plain_over_copy": round(plain[0] / copy[0], 3), "xform_over_copy": round(xf[0] / copy[0], 3),
               "xform_within_2x_of_copy": bool(xf[0] <= 2 * copy[0]),
               "xform_GBps_read_plus_write": round(2 * nbytes / (xf[0] * 1e-3) / 1e9, 1),
               "copy_GBps_read_plus_write": round(2 * nbytes / (copy[0] * 1e-3) / 1e9, 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def vgg11(torch, batch):
    import niti_amd
    from bench import synth_weights
    from niti_amd.model import NitiModel
    m = NitiModel(niti_amd.ARCH_VGG11, batch)
    m.keep_grads(False)
    for i, (w, s) in enumerate(synth_weights(m.layers, seed=17)):
        m.set_weight(i, w, s)
    return m


def bench_loop(torch, steps, rounds, autotune):
    from niti_amd import DeviceDataset, make_order
    batch = 256
    m = vgg11(torch, batch)
    count = steps * batch
    g = torch.Generator(device="cuda").manual_seed(3)
    data = torch.randint(0, 256, (count, 3, 32, 32), dtype=torch.uint8, device="cuda", generator=g)
    labels = torch.randint(0, 10, (count,), dtype=torch.int32, device="cuda", generator=g)
    ds = DeviceDataset(data, labels)
    x, lb = data[:batch].contiguous(), labels[:batch].contiguous()
    m.train_step_images(x, lb)
    if autotune:
        m.autotune()
    index, xform = make_order(count, batch, seed=2, epoch=0, pad=4, flip=True)
    ds.set_order(index, xform)
    for _ in range(20):
        m.train_step_images(x, lb)
    m.train_steps(ds, 0, 20)
    torch.cuda.synchronize()
    res = {"dataset": [], "resident": [], "dataset_metrics": []}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    def resident():
        for _ in range(steps):
            m.train_step_images(x, lb)

    for _ in range(rounds):
        res["dataset"].append(timed(lambda: m.train_steps(ds, 0, steps)))
        res["resident"].append(timed(resident))
        m.train_metrics(True)
        res["dataset_metrics"].append(timed(lambda: m.train_steps(ds, 0, steps)))
        m.train_metrics(False)
    if m.rowconv_error() != 0:
        raise RuntimeError("a fused row-kernel grid barrier timed out: results invalid")
    med = {k: statistics.median(v) for k, v in res.items()}
    row = {"section": "loop", "model": "VGG-11 batch 256", "steps_per_window": steps, "rounds": rounds,
           "autotuned": autotune, "timing": "host clock around the enqueue and one device synchronise",
           "dataset_ms_per_step": round(med["dataset"], 4), "resident_ms_per_step": round(med["resident"], 4),
           "difference_ms": round(med["dataset"] - med["resident"], 4),
           "dataset_with_metrics_ms_per_step": round(med["dataset_metrics"], 4),
           "dataset_images_per_s": round(batch / med["dataset"] * 1e3),
           "all_ms": {k: [round(v, 4) for v in vs] for k, vs in res.items()}}
    print(json.dumps(row), flush=True)
    # evaluation throughput, on the same model and the first 50 batches
    n = min(count, 50 * batch) - 3  # (a padded tail)
    eds = DeviceDataset(data[:n], labels[:n])
    m.evaluate_dataset(eds)
    m.evaluate(data[:n], labels[:n])
    ev = {"dataset": [], "tensors": []}
    for _ in range(rounds):
        for key, fn in (("dataset", lambda: m.evaluate_dataset(eds)), ("tensors", lambda: m.evaluate(data[:n], labels[:n]))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ev[key].append(time.perf_counter() - t0)
    erow = {"section": "eval", "model": "VGG-11 batch 256", "images": n,
            "evaluate_dataset_images_per_s": round(n / statistics.median(ev["dataset"])),
            "evaluate_images_per_s": round(n / statistics.median(ev["tensors"])),
            "evaluate_dataset_ms_per_batch": round(statistics.median(ev["dataset"]) / ((n + batch - 1) // batch) * 1e3, 4),
            "evaluate_ms_per_batch": round(statistics.median(ev["tensors"]) / ((n + batch - 1) // batch) * 1e3, 4)}
    print(json.dumps(erow), flush=True)
    return row, erow


def bench_resize(torch, reps):
    from niti_amd import DeviceDataset, center_windows, make_order, make_rrc_order
    rows = []
    for n, c, sh, sw, oh, ow, kind in ((128, 3, 256, 256, 224, 224, "rrc"), (128, 3, 256, 256, 224, 224, "centre"),
                                       (256, 3, 40, 40, 32, 32, "rrc")):
        count = 4 * n
        g = torch.Generator(device="cuda").manual_seed(n + sh)
        data = torch.randint(0, 256, (count, c, sh, sw), dtype=torch.uint8, device="cuda", generator=g)
        labels = torch.randint(0, 10, (count,), dtype=torch.int32, device="cuda", generator=g)
        ds = DeviceDataset(data, labels, out_hw=(oh, ow))
        index, xform, windows = make_rrc_order(count, n, seed=1, epoch=0, h=sh, w=sw)
        if kind == "centre":
            windows = center_windows(len(index), sh, sw, fraction=(oh / sh, ow / sw))
        ds.set_order(index, xform, windows)
        out = torch.empty((n, c, oh, ow), dtype=torch.uint8, device="cuda")
        lab = torch.empty(n, dtype=torch.int32, device="cuda")
        steps = len(index) // n
        k = [0]

        def gather(d=ds):
            d.gather((k[0] % steps) * n, n, out, lab)
            k[0] += 1

        rs = event_ms(torch, gather, reps)
        # the transformed gather at the same output shape: stored images of the output size
        same = DeviceDataset(data[:, :, :oh, :ow].contiguous(), labels)
        same.set_order(*make_order(count, n, seed=1, epoch=0, pad=4, flip=True))
        xf = event_ms(torch, lambda: gather(same), reps)
        # the copy: window bytes read + output bytes written per batch, moved by a copy of half as many
        read = int(c * (windows[:, 2].astype(np.int64) * windows[:, 3]).sum() // steps)
        written = n * c * oh * ow
        half = (read + written) // 2
        src = data.view(-1)[:half]
        dst = torch.empty(half, dtype=torch.uint8, device="cuda")
        copy = event_ms(torch, lambda: dst.copy_(src), reps)
        row = {"section": "resize", "shape": f"{n}x{c}x{oh}x{ow} from {sh}x{sw}", "windows": kind,
               "window_bytes_read": read, "output_bytes_written": written, "copy_bytes": half,
               "launches_per_window": reps,
               "resize_us": round(rs[0] * 1e3, 2), "xform_us": round(xf[0] * 1e3, 2), "copy_us": round(copy[0] * 1e3, 2),
               "resize_us_min": round(rs[1] * 1e3, 2), "xform_us_min": round(xf[1] * 1e3, 2),
               "copy_us_min": round(copy[1] * 1e3, 2),
               "resize_over_copy": round(rs[0] / copy[0], 3), "resize_over_xform": round(rs[0] / xf[0], 3),
               "resize_within_2x_of_copy": bool(rs[0] <= 2 * copy[0]),
               "resize_GBps_read_plus_write": round((read + written) / (rs[0] * 1e-3) / 1e9, 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def bench_resize_loop(torch, steps, rounds, autotune):
    """ResNet-18, batch 128, 224 px: fit_epoch-style dataset steps with random-resized-crop from
    256x256 stored images against train_step_images on one resident batch."""
    import niti_amd
    from bench import synth_weights
    from niti_amd import DeviceDataset, make_rrc_order
    from niti_amd.model import NitiModel
    batch = 128
    m = NitiModel(niti_amd.ARCH_RESNET18, batch)
    m.keep_grads(False)
    for i, (w, s) in enumerate(synth_weights(m.layers, seed=17)):
        m.set_weight(i, w, s)
    count = steps * batch
    g = torch.Generator(device="cuda").manual_seed(5)
    data = torch.randint(0, 256, (count, 3, 256, 256), dtype=torch.uint8, device="cuda", generator=g)
    labels = torch.randint(0, 1000, (count,), dtype=torch.int32, device="cuda", generator=g)
    ds = DeviceDataset(data, labels, out_hw=(224, 224))
    x, lb = data[:batch, :, 16:240, 16:240].contiguous(), labels[:batch].contiguous()
    m.train_step_images(x, lb)
    if autotune:
        m.autotune()
    ds.set_order(*make_rrc_order(count, batch, seed=2, epoch=0, h=256, w=256))
    for _ in range(5):
        m.train_step_images(x, lb)
    m.train_steps(ds, 0, 5)
    torch.cuda.synchronize()
    res = {"dataset": [], "resident": []}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    def resident():
        for _ in range(steps):
            m.train_step_images(x, lb)

    for _ in range(rounds):
        res["dataset"].append(timed(lambda: m.train_steps(ds, 0, steps)))
        res["resident"].append(timed(resident))
    if m.rowconv_error() != 0:
        raise RuntimeError("a fused row-kernel grid barrier timed out: results invalid")
    med = {k: statistics.median(v) for k, v in res.items()}
    row = {"section": "resize_loop", "model": "ResNet-18 batch 128, 224 px from 256x256 stored, random-resized-crop",
           "steps_per_window": steps, "rounds": rounds, "autotuned": autotune,
           "timing": "host clock around the enqueue and one device synchronise",
           "dataset_ms_per_step": round(med["dataset"], 4), "resident_ms_per_step": round(med["resident"], 4),
           "difference_ms": round(med["dataset"] - med["resident"], 4),
           "dataset_images_per_s": round(batch / med["dataset"] * 1e3),
           "all_ms": {k: [round(v, 4) for v in vs] for k, vs in res.items()}}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gather-reps", type=int, default=500, help="back-to-back launches per timed window")
    ap.add_argument("--loop-steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-autotune", action="store_true")
    ap.add_argument("--skip", default="", help="comma list of sections to skip: gather, loop, resize, resize_loop")
    ap.add_argument("--resize-loop-steps", type=int, default=24)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("dataset_bench.py measures on a GPU; none is visible")
    import niti_amd  # noqa: F401
    skip = set(args.skip.split(","))
    out = {}
    if "gather" not in skip:
        out["gather"] = bench_gather(torch, args.gather_reps)
    if "loop" not in skip:
        out["loop"], out["eval"] = bench_loop(torch, args.loop_steps, args.rounds, not args.no_autotune)
    if "resize" not in skip:
        out["resize"] = bench_resize(torch, args.gather_reps)
    if "resize_loop" not in skip:
        out["resize_loop"] = bench_resize_loop(torch, args.resize_loop_steps, args.rounds, not args.no_autotune)
    print(json.dumps({"dataset_bench": out}), flush=True)


if __name__ == "__main__":
    main()
