"""Per-phase stamp report of one item of wgrad_p16_many_kernel in its two forms (NITI_WG_STAMPS build,
tools/wg_diag_build.sh; NITI_HIP_LIB names the library): one job, one item per workgroup, so the
stamps a block leaves are that item's.  Prints mean cycles of prologue / K loop / LDS write (and, merged
form, the wait for the slowest wave and the sum) / output for the merged form (threshold 0, a tile per
workgroup) and the quad form (four tiles per workgroup).

usage: wg_quad_diag.py [layer of tools/wg_bench.py, default conv7]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mandheling-dsp-training_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import niti_amd._lib as L  # noqa: E402
from niti_amd import ops  # noqa: E402
from wg_bench import LAYERS  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "conv7"
    n, ci, h, co = LAYERS[name]
    rng = np.random.default_rng(0)
    g = ops.geom(n, ci, h, h, co, 3, stride=1, pad=1)
    x16 = torch.from_numpy(rng.integers(-127, 128, (n, h, h, ci), dtype=np.int16).astype(np.int8)).cuda()
    d16 = torch.from_numpy(rng.integers(-127, 128, (n, h, h, co), dtype=np.int16).astype(np.int8)).cuda()
    xP, dP = ops.nhwc16_to_p16(x16), ops.nhwc16_to_p16(d16)
    kg = n * h * h // 32
    tiles = (co // 32) * (ci // 32)
    lib = L.lib()
    outs = []
    try:
        for quad, blocks in ((0, tiles), (kg, (tiles + 3) // 4)):
            lib.niti_diag_wgrad_quad(quad)
            amax = ops.new_range()
            for _ in range(2):
                ops.conv_wgrad_p16_many([(g, xP, dP, amax)], blocks, 4 * kg)
            torch.cuda.synchronize()
            st = torch.zeros(blocks * 16, dtype=torch.int64, device="cuda")
            lib.niti_diag_wgrad_stamps(st.data_ptr())
            accs, splits = ops.conv_wgrad_p16_many([(g, xP, dP, amax)], blocks, 4 * kg)
            torch.cuda.synchronize()
            lib.niti_diag_wgrad_stamps(None)
            outs.append(accs[0])
            a = st.cpu().numpy().astype(np.int64)[:blocks * 8].reshape(-1, 8)
            assert splits == [1] and (a[:, 5] > a[:, 0]).all()
            d = np.diff(a[:, :6], axis=1).astype(np.float64)
            m, md = d.mean(0), np.median(d, axis=0)
            clk = np.median((a[:, 5] - a[:, 0]) / np.maximum(a[:, 7] - a[:, 6], 1) * 100.0)
            print(f"{name} {'quad' if quad else 'merged'} form: {blocks} workgroups x 1 item, {kg} K groups per tile; "
                  f"cycles mean (median): prologue {m[0]:.0f} ({md[0]:.0f}) K loop {m[1]:.0f} ({md[1]:.0f}) "
                  f"LDS write{'' if quad else ' + slowest wave'} {m[2]:.0f} ({md[2]:.0f}) sum {m[3]:.0f} ({md[3]:.0f}) "
                  f"output {m[4]:.0f} ({md[4]:.0f}) whole item {d.sum(1).mean():.0f}; clock {clk:.0f} MHz", flush=True)
    finally:
        lib.niti_diag_wgrad_quad(-1)
        lib.niti_diag_wgrad_stamps(None)
    assert torch.equal(outs[0], outs[1])


if __name__ == "__main__":
    main()
