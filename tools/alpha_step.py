"""Measurement aid (GPU box): what the accumulated-alpha image costs on BASELINE configs[3] (B = 1, 131 072 Gaussians, 3 views of
256 x 256, colour + built-in depth, through the plan API) - forward and training step (forward announced with
GSR_FLAG_BACKWARD_FOLLOWS + backward) with alpha off (gsr_forward_ex / gsr_backward_ex), with alpha on (the same calls with
out_alpha / dL_dalpha_img in their options), and the two-pass alternative alpha replaces: the same call followed by a second forward that
blends an `extra` array of ones (which cannot share a pass with the depth channel).  The variants are alternated repeat by repeat.
usage: python tools/alpha_step.py [steps per repeat = 200] [repeats = 5] [out.json]"""
import json
import os
import statistics
import sys
import time
from dataclasses import replace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd import _lib, synthetic  # noqa: E402
from pf3plat_amd.rasterizer import HipBackend, RasterConfig  # noqa: E402

H = W = 256
N, V = 131072, 3


def timed(step, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    if not torch.cuda.is_available():
        raise SystemExit("alpha_step.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    be = HipBackend()
    sc = synthetic.make_scene(50, N, (H, W), num_views=V)
    ins = tuple(t.to(dev).contiguous() for t in synthetic.scene_operator_inputs(sc))
    vb = synthetic.scene_viewbuf(sc).to(dev)
    gc, ge, ga = torch.rand((V, 3, H, W), device=dev), torch.rand((V, H, W), device=dev), torch.rand((V, H, W), device=dev)
    ones = torch.ones((V, N), device=dev)
    variants = {}
    for train in (False, True):
        fl = (_lib.FLAG_BACKWARD_FOLLOWS if train else 0) | (1 << 4)
        base = RasterConfig(V, 1, V, N, H, W, 4, 25, 4, True, fl)
        sizing = be.make_plan(base, dev, capacity=8 * V * N)
        be.run_forward(sizing, vb, *ins)
        cap = be.capacity_for(base, be.read_status(sizing), headroom=1.1)
        off = be.make_plan(base, dev, capacity=cap, backward=train)
        on = be.make_plan(replace(base, alpha=True), dev, capacity=cap, backward=train)
        second = be.make_plan(replace(base, flags=0), dev, capacity=cap)  # the second pass of the alternative: extra = ones, forward only

        def step_off(off=off, train=train):
            be.run_forward(off, vb, *ins)
            if train:
                be.run_backward(off, vb, *ins, None, gc, ge)

        def step_on(on=on, train=train):
            be.run_forward(on, vb, *ins)
            if train:
                be.run_backward(on, vb, *ins, None, gc, ge, g_alpha_img=ga)

        def step_two(off=off, second=second, train=train):
            be.run_forward(second, vb, *ins, ones)
            step_off(off, train)

        kind = "train" if train else "fwd"
        variants.update({f"{kind}_alpha_off": step_off, f"{kind}_alpha_on": step_on, f"{kind}_second_pass_of_ones": step_two})
        step_on()
        step_two()
        torch.cuda.synchronize()
        assert not be.read_status(on)["overflow"] and not be.read_status(second)["overflow"]
        # the alternative's image is the same quantity (to rounding: sum alpha T against 1 - T)
        assert float((on["alpha_img"] - second["extra_img"]).abs().max()) < 1e-4
    for fn in variants.values():  # warm-up: clocks, allocator, code objects
        for _ in range(50):
            fn()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():  # alternated: drift of the machine hits all of them
            times[k].append(timed(fn, steps))
    out = {"shape": f"1 scene x {N} Gaussians (seed 50, degree 4), {V} views {H}x{W}, colour + built-in depth, plan API", "steps_per_repeat": steps,
           "repeats": repeats, "us_per_call": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                               for k, v in times.items()}}
    print(json.dumps(out))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
