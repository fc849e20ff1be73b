"""Adapter -> decoder training step at PF3plat's training batch, harmonics rotated by torch (`rotate_sh`, the default adapter)
against harmonics left in their source camera's frame and rotated in the raster kernels (GaussianAdapter(fuse_sh_rotation=True),
GSR_FLAG_SH_IN_FRAME), and against that with the adapter itself compiled as well (GaussianAdapter(fuse_sh_rotation=True,
fused=True): gsr_adapt / gsr_adapt_backward, one launch each way, the same inputs).  Shape: 4 scenes x 2 source views x 256^2 pixel-aligned Gaussians (131 072 per scene, degree 4), 3 target
views of 256^2 per scene, colour + depth loss, forward + backward.  HIP events around each step, warm-up first, the three forms
alternated call by call; reports median and spread of the repeats and torch.cuda.max_memory_allocated of one step of each.
usage (GPU box): python tools/adapter_step.py [steps per repeat] [repeats] [out.json]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pf3plat_amd  # noqa: E402
from pf3plat_amd import synthetic  # noqa: E402
from pf3plat_amd.adapter import GaussianAdapter, GaussianAdapterCfg  # noqa: E402

B, HS, WS, HW = 4, 256, 256, (256, 256)


def inputs(dev):
    g = torch.Generator().manual_seed(3)
    ext = torch.eye(4).repeat(B, 2, 1, 1)
    for b in range(B):
        for v, x in enumerate((-0.5, 0.5)):
            a = 0.1 * (torch.rand(3, generator=g) - 0.5)  # a few degrees about each axis: proper, non-trivial frames
            k = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            ext[b, v, :3, :3] = torch.linalg.matrix_exp(k)
            ext[b, v, 0, 3] = x
    intr = torch.tensor([[0.86, 0, 0.5], [0, 0.86, 0.5], [0, 0, 1]]).repeat(B, 2, 1, 1)
    yy, xx = torch.meshgrid((torch.arange(HS) + 0.5) / HS, (torch.arange(WS) + 0.5) / WS, indexing="ij")
    coords = torch.stack((xx, yy), -1).reshape(1, 1, HS * WS, 2).expand(B, 2, HS * WS, 2).contiguous()
    depths = 3.0 + torch.sin(6 * xx + 2 * yy).reshape(1, 1, HS * WS) + 0.02 * torch.rand((B, 2, HS * WS), generator=g)
    opac = 0.1 + 0.85 * torch.rand((B, 2, HS * WS), generator=g)
    raw = torch.randn((B, 2, HS * WS, 82), generator=g)
    sc = synthetic.make_scene(50, 8, HW, num_views=3)
    cams = [x.expand(B, *x.shape[1:]).contiguous() for x in (sc.extrinsics, sc.intrinsics, sc.near, sc.far)]
    w = torch.rand((B, 3, 3, *HW), generator=g)
    wd = 0.05 * torch.rand((B, 3, *HW), generator=g)
    return [x.to(dev) for x in (ext[:, :, None], intr[:, :, None], coords, depths, opac, raw, w, wd)], [c.to(dev) for c in cams]


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    if not torch.cuda.is_available():
        raise SystemExit("adapter_step.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    (ext, intr, coords, depths, opac, raw0, w, wd), cams = inputs(dev)
    cfg = GaussianAdapterCfg(0.5, 15.0, 4)
    adapters = {"torch_rotation": GaussianAdapter(cfg).to(dev), "fused": GaussianAdapter(cfg, fuse_sh_rotation=True).to(dev),
                "hip_adapter": GaussianAdapter(cfg, fuse_sh_rotation=True, fused=True).to(dev)}
    dec = pf3plat_amd.DecoderSplattingCUDA().to(dev)
    raw = raw0.clone().requires_grad_(True)

    def step(name):
        raw.grad = None
        g = adapters[name].forward(ext, intr, coords, depths, opac, raw, HW).for_decoder()
        o = dec.forward(g, *cams, HW, depth_mode="depth")
        ((o.color * w).sum() + (o.depth * wd).sum()).backward()
        return o

    # same results first (the measurement is of two forms of ONE computation)
    res = {}
    for name in adapters:
        o = step(name)
        res[name] = (o.color.detach().clone(), o.depth.detach().clone(), raw.grad.detach().clone())
    assert adapters["hip_adapter"].last_path == "hip" and adapters["fused"].last_path == "torch"
    rel = lambda a, b: float((a - b).double().norm() / b.double().norm())
    agree = {k: rel(res["fused"][i], res["torch_rotation"][i]) for i, k in enumerate(("color", "depth", "d_raw"))}
    agree_hip = {k: rel(res["hip_adapter"][i], res["fused"][i]) for i, k in enumerate(("color", "depth", "d_raw"))}
    mem = {}
    for name in adapters:
        for _ in range(3):
            step(name)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        step(name)
        torch.cuda.synchronize()
        mem[name] = {"max_memory_allocated_MB": torch.cuda.max_memory_allocated(dev) / 2**20, "resident_before_MB": base / 2**20}
    times = {k: [] for k in adapters}
    for _ in range(repeats):
        for name in adapters:  # alternated: drift of the machine hits both
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step(name)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / steps)
    summary = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 4) for x in v]}
               for k, v in times.items()}
    out = {"shape": f"{B} scenes x 2 x {HS}x{WS} Gaussians (131072 per scene, degree 4), 3 target views {HW}, colour + depth, fwd + bwd",
           "steps_per_repeat": steps, "repeats": repeats, "time": summary, "memory": mem, "fused_vs_torch_rel_l2": agree,
           "hip_adapter_vs_fused_rel_l2": agree_hip, "saving_ms": summary["torch_rotation"]["median_ms"] - summary["fused"]["median_ms"],
           "hip_adapter_saving_ms": summary["fused"]["median_ms"] - summary["hip_adapter"]["median_ms"]}
    print(json.dumps(out))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
