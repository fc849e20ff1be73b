"""Measurement aid (GPU box), sibling of tools/pose_loss_prof.py: the encoder's plane-sweep cost volume (gsr_cost_volume /
gsr_cost_volume_backward through pf3plat_amd.cost_volume.plane_sweep_cost_volume) next to the torch form the reference evaluates it
in (tests/cost_volume_ref.cost_volume_torch_form: `F.grid_sample` into the warped features (b, c, D, h, w) per other view, a product
and a sum over c) on the SAME device, in ONE process and alternating blocks, so that both see the same machine.  Shapes: the
training batch (14, 2, 256, 64, 64, 128) and the evaluation shape (1, 2, 256, 64, 64, 128); if the torch form does not fit at 14
scenes it is timed at the largest scene count that does, and the line says so.  Figures, each the wall time per call of a host clock
around `reps` calls that end in a synchronise: the forward (under no_grad) and the training step (forward + backward) of both forms,
and each form's torch.cuda.max_memory_allocated over one step on top of what was allocated before it.  Before timing, the two
forms' values and gradients are compared.
usage: python tools/cost_volume_prof.py [reps=20] [rounds=5] [torch_reps=3]"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd.cost_volume import plane_sweep_cost_volume  # noqa: E402
from tests import cost_volume_ref as ref  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
torch_reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
dev = torch.device("cuda:0")


def timed(fn, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / count


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


def measure(label, b, torch_b):
    v, c, h, w, d = 2, 256, 64, 64, 128
    case = ref.build_case(0, b, v, c, h, w, 1, 0.1)  # (the cotangent of this call is not used: it would be made on the host)
    feats, intr, extr, near, far = (case[k].to(dev) for k in ("features", "intrinsics", "extrinsics", "near", "far"))
    cot = torch.randn(v * b, d, h, w, device=dev)
    tb = torch_b

    def hip_fwd():
        with torch.no_grad():
            return plane_sweep_cost_volume(feats, intr, extr, near, far, d)

    def hip_step():
        f = feats.detach().requires_grad_(True)
        plane_sweep_cost_volume(f, intr, extr, near, far, d).backward(cot)
        return f.grad

    def torch_fwd():
        with torch.no_grad():
            return ref.cost_volume_torch_form(feats[:tb], intr[:tb], extr[:tb], near[:tb], far[:tb], d)

    def torch_step():
        f = feats[:tb].detach().requires_grad_(True)
        ref.cost_volume_torch_form(f, intr[:tb], extr[:tb], near[:tb], far[:tb], d).backward(cot.view(v, b, d, h, w)[:, :tb].reshape(v * tb, d, h, w))
        return f.grad

    print(f"--- {label}: (b, v, c, h, w, D) = ({b}, {v}, {c}, {h}, {w}, {d}); the torch form at b = {tb}"
          + ("" if tb == b else f" (the largest that was tried to fit; its times are NOT scaled to b = {b})"))
    a, t = hip_fwd().view(v, b, d, h, w)[:, :tb], torch_fwd().view(v, tb, d, h, w)
    print(f"value: rel-L2 hip vs torch form {float((a - t).norm() / t.norm()):.2e}; exactly zero share {float((t == 0).float().mean()):.3f}")
    ga, gt = hip_step()[:tb], torch_step()
    print(f"dL/dfeatures: rel-L2 hip vs torch form {float((ga - gt).norm() / gt.norm()):.2e}" + ("" if tb == b else "  (scenes are independent)"))
    del a, t, ga, gt
    legs = {"HIP    forward": (hip_fwd, reps), "HIP    forward + backward": (hip_step, reps),
            "torch  forward": (torch_fwd, torch_reps), "torch  forward + backward": (torch_step, torch_reps)}
    for name, (fn, _) in legs.items():
        print(f"{name:28s} peak memory over one call {peak(fn):10.1f} MB")
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, (fn, count) in legs.items():
            times[name].append(timed(fn, count))
    med = {}
    for name, ts in times.items():
        med[name] = sorted(ts)[len(ts) // 2]
        print(f"{name:28s} median {med[name]:9.3f} ms   min {min(ts):9.3f}   max {max(ts):9.3f}   ({rounds} x {legs[name][1]} calls)")
    scale = b / tb
    print(f"ratio torch / HIP: forward {med['torch  forward'] * scale / med['HIP    forward']:.2f}, "
          f"step {med['torch  forward + backward'] * scale / med['HIP    forward + backward']:.2f}"
          + ("" if tb == b else f"  (torch times x {scale:.2f} for the scene count: scenes are independent)"))


def fits(b):
    try:
        case = ref.build_case(0, b, 2, 256, 64, 64, 1, 0.1)
        args = [case[k].to(dev) for k in ("features", "intrinsics", "extrinsics", "near", "far")]
        f = args[0].requires_grad_(True)
        ref.cost_volume_torch_form(f, *args[1:], 128).sum().backward()
        torch.cuda.synchronize()
        return True
    except torch.cuda.OutOfMemoryError:
        return False
    finally:
        torch.cuda.empty_cache()


measure("evaluation", 1, 1)
tb = next((b for b in (14, 7, 4, 2, 1) if fits(b)), 1)
measure("training", 14, tb)
