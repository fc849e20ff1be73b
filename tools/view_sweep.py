"""Measurement aid (GPU box): consecutive single-view forwards of ONE scene through ONE plan while the camera moves a little
between calls - what the tile launch's deal (gsr_common.h: build_tile_order) sees in real use, where its hint, the previous call's
walked counts, is close but not exact.  Printed beside the identical-frame loop (the benchmark's headline: the hint is exact) and
beside a loop that alternates two far-apart cameras (every hint from another view).

usage: python tools/view_sweep.py [--gaussians 300000] [--views 64] [--step 0.004] [--passes 20] [--windows 5]
One JSON line: us per call, median over the windows, for the three loops, and how much the walked counts change between neighbours."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pf3plat_amd import synthetic  # noqa: E402
from pf3plat_amd.rasterizer import HipBackend, RasterConfig  # noqa: E402

H = W = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=300000)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--step", type=float, default=0.004, help="camera shift along x between consecutive calls (the source cameras sit at +-0.5)")
    ap.add_argument("--passes", type=int, default=20, help="sweeps (there and back) per timed window")
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, K = a.gaussians, a.views
    offs = [(k - (K - 1) / 2) * a.step for k in range(K)]
    sc = synthetic.make_scene(2, n, (H, W), d_sh=25, num_views=K, view_offsets=offs)
    ins = tuple(t.to(dev).contiguous() for t in synthetic.scene_operator_inputs(sc))
    vbs = synthetic.scene_viewbuf(sc).to(dev)
    cfg = RasterConfig(1, 1, 1, n, H, W, 4, 25, 4, False)
    be = HipBackend()
    plan = be.make_plan(cfg, dev, capacity=8 * n)
    worst = dict(num_pairs=0, max_list=0)
    for k in (0, K // 2, K - 1):
        be.run_forward(plan, vbs[k:k + 1].contiguous(), *ins)
        st = be.read_status(plan)
        worst = {q: max(worst[q], int(st[q])) for q in worst}
    plan = be.make_plan(cfg, dev, capacity=be.capacity_for(cfg, worst, headroom=1.2))
    views = [vbs[k:k + 1].contiguous() for k in range(K)]
    calls = [be.bind_forward(plan, v, *ins) for v in views]
    there_and_back = list(range(K)) + list(range(K - 2, 0, -1))
    loops = {"identical_frame": [K // 2] * len(there_and_back), "sweep": there_and_back,
             "two_far_views": [0 if i % 2 else K - 1 for i in range(len(there_and_back))]}
    lay = be.workspace_layout(plan["dims"])
    walked = []
    for k in (K // 2, K // 2 + 1, K - 1):
        calls[k]()
        torch.cuda.synchronize()
        walked.append(plan["bin"][lay["tile_total"]: lay["tile_total"] + 4096].view(torch.int32).cpu().double())
    cc = lambda x, y: round(torch.corrcoef(torch.stack([x, y]))[0, 1].item(), 4)
    out = dict(gaussians=n, views=K, step=a.step, overflow=int(be.read_status(plan)["overflow"]),
               walked_corr_neighbour=cc(walked[0], walked[1]), walked_corr_far=cc(walked[0], walked[2]))
    for name, order in loops.items():
        for k in order:  # warm-up: one pass
            calls[k]()
        torch.cuda.synchronize()
        meds = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.passes):
                for k in order:
                    calls[k]()
            e1.record()
            torch.cuda.synchronize()
            meds.append(e0.elapsed_time(e1) * 1e3 / (a.passes * len(order)))
        out[name + "_us"] = round(statistics.median(meds), 3)
        out[name + "_us_windows"] = [round(m, 3) for m in meds]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
