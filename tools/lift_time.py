"""Measurement aid (GPU box; fails without a device): the encoder's depth lift (pf3plat_amd.lift.lift_depth: gsr_lift_depth /
gsr_lift_depth_backward) and the Pluecker ray map (plucker_rays) next to the same arithmetic as eager torch ops on the SAME device -
the float32 form of tests/lift_ref.py (refined_depth, points, mono_cue, plucker), which is not the code under test.  At PF3plat's
size: 4 scenes x 3 views, 256 x 256, D = 128; the ray map at 64 x 64.  Legs: the forward (no_grad), the training step (forward +
backward for cotangents on depth and xyz, gradients to depth_raw and shift) and the ray map, of both forms.  After a warm-up the legs
alternate in one process; a window is `iters` calls between two device events and ends in a synchronise; `repeats` windows per leg.
Printed per leg: the median time per call, the spread (min .. max) over the repeats, the launches one call makes (counted with
torch.profiler, in a pass of their own after the timing), the bytes the algorithm needs - computed from the shapes: one read of
depth_raw and shift, one write of depth, xyz and the cue; the step adds one read of the inputs and the cotangents and one write of the
two gradients - and the fraction of 8 TB/s those bytes imply at the measured time.
usage: python tools/lift_time.py [iters=200] [repeats=5]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd.lift import lift_depth, plucker_rays  # noqa: E402
from tests import lift_ref as ref  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
if not torch.cuda.is_available():
    sys.exit("tools/lift_time.py measures on the GPU: no device found")
dev = torch.device("cuda:0")
B, V, H, W, D, HQ = 4, 3, 256, 256, 128, 64
PEAK = 8e12  # bytes per second


def algorithmic_bytes():
    n, cue = B * V * H * W, B * V * D * (H // 4) * (W // 4)
    fwd = 4 * (2 * n + 4 * n + cue)             # read depth_raw, shift; write depth, xyz, cue
    bwd = 4 * (2 * n + 4 * n + 2 * n)           # read depth_raw, shift, dL/ddepth, dL/dxyz; write dL/ddepth_raw, dL/dshift
    rays = 4 * B * V * 6 * HQ * HQ
    return {"forward": fwd, "step": fwd + bwd, "rays": rays}


def window(fn, count):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(count):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return 1e3 * start.elapsed_time(stop) / count  # microseconds per call


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as e:  # noqa: BLE001
        return f"not counted ({type(e).__name__})"


def main():
    case = ref.build_case(0, B, V, H, W, D)
    raw, shift, near, far, K, c2w, g_depth, g_xyz = (case[k].to(dev) for k in ("depth_raw", "shift", "near", "far", "intrinsics", "c2w", "g_depth", "g_xyz"))

    def hip_fwd():
        with torch.no_grad():
            return lift_depth(raw, shift, near, far, K, D)

    def torch_fwd():
        with torch.no_grad():
            depth, xyz = ref.lift(raw, shift, near, far, K)
            return depth, xyz, ref.mono_cue(depth, near, far, D)

    def hip_step():
        r, s = raw.detach().requires_grad_(True), shift.detach().requires_grad_(True)
        out = lift_depth(r, s, near, far, K, D)
        torch.autograd.backward([out.depth, out.xyz], [g_depth, g_xyz])
        return r.grad, s.grad, out.mono_cue

    def torch_step():
        r, s = raw.detach().requires_grad_(True), shift.detach().requires_grad_(True)
        depth, xyz = ref.lift(r, s, near, far, K)
        cue = ref.mono_cue(depth, near, far, D)
        torch.autograd.backward([depth, xyz], [g_depth, g_xyz])
        return r.grad, s.grad, cue

    hip_rays = lambda: plucker_rays(c2w, K, (HQ, HQ))
    torch_rays = lambda: ref.plucker(c2w, K, HQ, HQ)

    # the two forms compute the same thing at this size
    a, t = hip_fwd(), torch_fwd()
    same = float((a.mono_cue == t[2]).float().mean())
    print(f"value: depth bit-equal {torch.equal(a.depth, t[0])}, xyz rel-L2 {ref.rel_l2(a.xyz, t[1]):.2e}, cue entries equal {same:.6f}")
    ga, gt = hip_step(), torch_step()
    print(f"gradients: d_depth_raw rel-L2 {ref.rel_l2(ga[0], gt[0]):.2e}, d_shift {ref.rel_l2(ga[1], gt[1]):.2e}; ray map {ref.rel_l2(hip_rays(), torch_rays()):.2e}")
    del a, t, ga, gt

    legs = {"HIP   forward": (hip_fwd, "forward"), "torch forward": (torch_fwd, "forward"), "HIP   step": (hip_step, "step"),
            "torch step": (torch_step, "step"), "HIP   rays 64 x 64": (hip_rays, "rays"), "torch rays 64 x 64": (torch_rays, "rays")}
    for fn, _ in legs.values():  # warm-up: code objects, the allocator, every shape of the timed windows
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(repeats):
        for name, (fn, _) in legs.items():
            times[name].append(window(fn, iters))
    need = algorithmic_bytes()
    med = {}
    print(f"(b, v, h, w, D) = ({B}, {V}, {H}, {W}, {D}); {repeats} windows of {iters} calls per leg, alternating; microseconds per call")
    for name, (fn, kind) in legs.items():
        ts = sorted(times[name])
        med[name] = ts[len(ts) // 2]
        print(f"{name:20s} median {med[name]:9.2f} us   min {ts[0]:9.2f}   max {ts[-1]:9.2f}   launches {launches(fn)}   "
              f"algorithmic {need[kind] / 1e6:7.2f} MB -> {need[kind] / (med[name] * 1e-6) / PEAK:6.1%} of 8 TB/s")
    for kind, h, t in (("forward", "HIP   forward", "torch forward"), ("step", "HIP   step", "torch step"), ("rays", "HIP   rays 64 x 64", "torch rays 64 x 64")):
        spread = max(max(times[h]) - min(times[h]), max(times[t]) - min(times[t]))
        print(f"{kind}: torch / HIP = {med[t] / med[h]:.2f}; difference {med[t] - med[h]:.2f} us against a spread of {spread:.2f} us")


if __name__ == "__main__":
    main()
