"""Adapter -> decoder training step at PF3plat's training batch with LEARNED source intrinsics (`intrinsics.requires_grad_()` on the
source cameras; inputs and shape of tools/adapter_step.py, harmonics left in their frames), three forms of the adapter:
  hip_intrinsics    GaussianAdapter(fused=True): gsr_adapt / gsr_adapt_backward_ex, dL/dintrinsics from the same two backward launches;
  torch_intrinsics  GaussianAdapter(fused=False): the torch ops - what a fused=True adapter ran for such a call before the compiled
                    backward had an intrinsics gradient;
  hip_plain         GaussianAdapter(fused=True) with intrinsics that do not require grad (tools/adapter_step.py's `hip_adapter` form:
                    the figure to hold against that tool's, same machine, same session).
HIP events around each step, warm-up first, the forms alternated call by call, one untimed step of a form in front of each of its
timed windows (the window then does not depend on which form ran before it); reports median and spread of the repeats.
usage (GPU box): python tools/adapter_intrinsics_step.py [steps per repeat] [repeats] [out.json]"""
import importlib.util
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pf3plat_amd  # noqa: E402
from pf3plat_amd.adapter import GaussianAdapter, GaussianAdapterCfg  # noqa: E402

_spec = importlib.util.spec_from_file_location("adapter_step", os.path.join(ROOT, "tools", "adapter_step.py"))
adapter_step = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(adapter_step)
inputs, HW = adapter_step.inputs, adapter_step.HW


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    if not torch.cuda.is_available():
        raise SystemExit("adapter_intrinsics_step.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    (ext, intr0, coords, depths, opac, raw0, w, wd), cams = inputs(dev)
    cfg = GaussianAdapterCfg(0.5, 15.0, 4)
    hip, ops = GaussianAdapter(cfg, fuse_sh_rotation=True, fused=True).to(dev), GaussianAdapter(cfg, fuse_sh_rotation=True).to(dev)
    forms = {"hip_intrinsics": (hip, True), "torch_intrinsics": (ops, True), "hip_plain": (hip, False)}
    dec = pf3plat_amd.DecoderSplattingCUDA().to(dev)
    raw = raw0.clone().requires_grad_(True)
    leaf = intr0.clone().requires_grad_(True)

    def step(name):
        adapter, learned = forms[name]
        raw.grad = leaf.grad = None
        g = adapter.forward(ext, leaf if learned else intr0, coords, depths, opac, raw, HW).for_decoder()
        o = dec.forward(g, *cams, HW, depth_mode="depth")
        ((o.color * w).sum() + (o.depth * wd).sum()).backward()
        return o

    # same results first (the measurement is of forms of ONE computation)
    res = {}
    for name, (adapter, learned) in forms.items():
        o = step(name)
        assert adapter.last_path == ("hip" if adapter.fused else "torch"), (name, adapter.last_path)
        assert (leaf.grad is not None) == learned, name
        res[name] = (o.color.detach().clone(), o.depth.detach().clone(), raw.grad.detach().clone(), leaf.grad.detach().clone() if learned else None)
    rel = lambda a, b: float((a - b).double().norm() / b.double().norm())
    what = ("color", "depth", "d_raw", "d_intrinsics")
    agree = {k: rel(res["hip_intrinsics"][i], res["torch_intrinsics"][i]) for i, k in enumerate(what)}
    same_bits = {k: bool(torch.equal(res["hip_intrinsics"][i], res["hip_plain"][i])) for i, k in enumerate(what[:2])}  # (the forward; the render's backward adds with atomics)
    for name in forms:
        for _ in range(3):
            step(name)
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(repeats):
        for name in forms:  # alternated: drift of the machine hits all
            step(name)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step(name)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / steps)
    summary = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 4) for x in v]}
               for k, v in times.items()}
    med = lambda k: summary[k]["median_ms"]
    out = {"shape": f"{adapter_step.B} scenes x 2 x {adapter_step.HS}x{adapter_step.WS} Gaussians (131072 per scene, degree 4), source intrinsics learned, "
                    f"3 target views {HW}, colour + depth, fwd + bwd",
           "steps_per_repeat": steps, "repeats": repeats, "time": summary, "hip_vs_torch_rel_l2": agree, "hip_intrinsics_vs_hip_plain_forward_same_bits": same_bits,
           "saving_ms": med("torch_intrinsics") - med("hip_intrinsics"), "intrinsics_gradient_cost_ms": med("hip_intrinsics") - med("hip_plain")}
    print(json.dumps(out))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
