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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gather-reps", type=int, default=500, help="back-to-back launches per timed window")
    ap.add_argument("--loop-steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-autotune", action="store_true")
    ap.add_argument("--skip", default="", help="comma list of sections to skip: gather, loop")
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
    print(json.dumps({"dataset_bench": out}), flush=True)


if __name__ == "__main__":
    main()
