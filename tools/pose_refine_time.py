"""Measurement aid (GPU box; fails without a device): the refined poses (pf3plat_amd.pose.refine_poses: gsr_pose_refine /
gsr_pose_refine_backward) next to the reference's eager lines in float32 on the SAME device - encoder_costvolume.py:447-450, 460-473
with its two `refine_sync_abspose.inverse()` calls (:492, :530) and the `c2w[1].inverse()` of model_wrapper.py:150, written anew
below; not the code under test.  At PF3plat's size: b = 4 scenes of v = 3 views, delta the first nine channels of a (b, v, 139) head
output, gamma a 0-dim parameter.  Legs: the forward (no_grad) and the training step (forward + backward for cotangents on c2w and on
the inverses, gradients to the head's output and to gamma) of both forms.  The operator is launch-bound: what is measured is the
host's cost of issuing the launches, the device being idle in between.  After a warm-up the legs alternate in one process; a
window is `iters` calls between two device events and ends in a synchronise; `repeats` windows per leg.  Printed per leg: the median
time per call, the spread (min .. max) over the repeats and the launches one call makes (counted with torch.profiler, in a pass of
their own after the timing).
usage: python tools/pose_refine_time.py [iters=20] [repeats=5]"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd.pose import refine_poses  # noqa: E402
from tests import pose_refine_ref as ref  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
if not torch.cuda.is_available():
    sys.exit("tools/pose_refine_time.py measures on the GPU: no device found")
dev = torch.device("cuda:0")
B, V = 4, 3


def eager(sync_abspose, delta, gamma):
    """The reference's lines as the training step runs them: the block, then its three inversions (two in the encoder, one in the
    model wrapper).  Returns c2w and the three inverses."""
    init_pose = sync_abspose
    raw_rot = init_pose[:, :, :3, :3][..., :2, :].clone().reshape(*init_pose.shape[:2], 6)
    raw_trans = init_pose[:, :, :3, 3]
    pred_pose_enc = torch.cat([raw_rot, raw_trans], dim=-1)
    delta_pred_pose_enc = delta[..., :9]
    pred_pose = pred_pose_enc[:, 1:] + delta_pred_pose_enc[:, 1:] * gamma
    pred_concat_pose = torch.cat([pred_pose_enc[:, :1], pred_pose], dim=1)
    d6 = pred_concat_pose[:, :, :6]
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = F.normalize(b2, dim=-1)
    b3 = torch.cross(b1, b2, dim=-1)
    rot6d = torch.stack((b1, b2, b3), dim=-2)
    trans3d = pred_concat_pose[:, :, 6:]
    Rt = torch.cat([rot6d, trans3d[..., None]], dim=-1)
    pad = torch.zeros_like(Rt[..., 2:3, :])
    pad[..., -1] = 1.0
    refine_sync_abspose = torch.cat((Rt, pad), dim=-2)
    return refine_sync_abspose, refine_sync_abspose.inverse(), refine_sync_abspose.inverse(), refine_sync_abspose.inverse()


def fused(sync_abspose, delta, gamma):
    out = refine_poses(sync_abspose, delta[..., :9], gamma)
    return out.c2w, out.w2c, out.w2c, out.w2c  # one inverse serves the three readers


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
    case = ref.build_case(0, B, V, "plain", 1.0)
    sync, full = case["sync"].to(dev), case["full"].to(dev)
    gamma = torch.tensor(case["gamma"], device=dev)
    cots = [case["cot_c2w"].to(dev), case["cot_w2c"].to(dev), 0.5 * case["cot_w2c"].to(dev), 0.25 * case["cot_w2c"].to(dev)]

    def forward(fn):
        def run():
            with torch.no_grad():
                return fn(sync, full, gamma)
        return run

    def step(fn):
        def run():
            f, g = full.detach().requires_grad_(True), gamma.detach().requires_grad_(True)
            outs = fn(sync, f, g)
            torch.autograd.backward(outs, cots)
            return f.grad, g.grad
        return run

    legs = {"HIP   forward": forward(fused), "torch forward": forward(eager), "HIP   step": step(fused), "torch step": step(eager)}
    # the two forms compute the same thing at this size
    a, t = legs["HIP   forward"](), legs["torch forward"]()
    ga, gt = legs["HIP   step"](), legs["torch step"]()
    print(f"c2w rel-L2 {ref.rel_l2(a[0], t[0]):.2e}, w2c {ref.rel_l2(a[1], t[1]):.2e}; gradients: head output {ref.rel_l2(ga[0], gt[0]):.2e}, "
          f"gamma {ref.rel_l2(ga[1], gt[1]):.2e}")
    for fn in legs.values():  # warm-up: code objects, the allocator, every shape of the timed windows
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            times[name].append(window(fn, iters))
    med = {}
    print(f"(b, v) = ({B}, {V}); {repeats} windows of {iters} calls per leg, alternating; microseconds per call")
    for name, fn in legs.items():
        ts = sorted(times[name])
        med[name] = ts[len(ts) // 2]
        print(f"{name:14s} median {med[name]:9.1f} us   min {ts[0]:9.1f}   max {ts[-1]:9.1f}   launches {launches(fn)}")
    for kind, h, t in (("forward", "HIP   forward", "torch forward"), ("step", "HIP   step", "torch step")):
        spread = max(max(times[h]) - min(times[h]), max(times[t]) - min(times[t]))
        print(f"{kind}: torch / HIP = {med[t] / med[h]:.2f}; difference {med[t] - med[h]:.1f} us against a spread of {spread:.1f} us")


if __name__ == "__main__":
    main()
