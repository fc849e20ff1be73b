"""Measurement aid (GPU box), sibling of tools/metrics_prof.py: the pose loss of the training step (gsr_pose_loss /
gsr_pose_loss_backward through pf3plat_amd.losses.pose_loss) next to the loop form the reference evaluates it in
(tests/pose_loss_ref.pose_loss_loop: whole-grid projections per pair, then a Python loop over the lists) on the SAME device, in ONE
process and alternating blocks, so that both see the same machine.  Shape: the shipped training batch, b = 14 scenes of v = 3 views of
256 x 256 pixels, about 1 000 matches per list (seeded, ragged: 600 .. 1 400).  Figures, each the wall time per call of a host clock
around `reps` calls that end in a synchronise: forward and forward + backward of both forms, the packing of the reference's
dict-of-lists, and the C ABI's forward and backward chains alone on preallocated buffers.  The launches of one call are counted
with torch's profiler (kernels and memsets on the device).  Before timing, the two forms' values and gradients are compared.
usage: python tools/pose_loss_prof.py [reps=200] [rounds=5] [loop_reps=20]"""
import ctypes
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd import _lib, losses  # noqa: E402
from pf3plat_amd.rasterizer import _stream_ptr  # noqa: E402
from tests import pose_loss_ref as ref  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
loop_reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
B, V, H, W = 14, 3, 256, 256
W2D, W3D = 1.0, 1.0
dev = torch.device("cuda:0")
lib = _lib.load()

g = torch.Generator().manual_seed(0)
lengths = torch.randint(600, 1401, (B * V * (V - 1) // 2,), generator=g).tolist()
sc = ref.build_scene(0, B, V, H, W, lengths, ["near" if s % 2 else "random" for s in range(B)])
xyz, depth, poses, intr = (t.to(dev) for t in (sc.xyz, sc.depth, sc.poses, sc.intrinsics))
corr = {p: [tuple(t.to(dev) for t in e) for e in lists] for p, lists in sc.corr.items()}
conf = {p: c.to(dev) for p, c in sc.conf.items()}
packed = losses.pack_correspondences(corr, conf)
print(f"b={B} v={V} {H}x{W}: {len(lengths)} lists, {packed.offsets[-1]} matches, "
      f"{lib.gsr_pose_loss_units(len(lengths), (ctypes.c_int32 * len(packed.offsets))(*packed.offsets))} units of 256")


def leaves():
    return tuple(t.clone().requires_grad_(True) for t in (xyz, depth, poses))


def hip_fwd():
    with torch.no_grad():
        return losses.pose_loss(xyz, depth, poses, intr, packed, W2D, W3D)[0]


def hip_fwd_bwd(x=None):
    x = x or leaves()
    losses.pose_loss(*x, intr, packed, W2D, W3D)[0].backward()
    return x


def hip_pack_fwd_bwd():
    x = leaves()
    losses.pose_loss(*x, intr, losses.pack_correspondences(corr, conf), W2D, W3D)[0].backward()


def loop_fwd():
    with torch.no_grad():
        return ref.pose_loss_loop(xyz, depth, poses, intr, corr, conf, W2D, W3D)[0]


def loop_fwd_bwd(x=None):
    x = x or leaves()
    ref.pose_loss_loop(*x, intr, corr, conf, W2D, W3D)[0].backward()
    return x


# the two forms compute the same thing (float32 both: the last digits differ)
a, b = hip_fwd_bwd(), loop_fwd_bwd()
print(f"value: hip {float(hip_fwd()):.6f}   loop {float(loop_fwd()):.6f}")
for name, p, q in zip(("xyz", "depth", "poses"), a, b):
    print(f"dL/d{name}: rel-L2 hip vs loop {float((p.grad - q.grad).norm() / q.grad.norm()):.2e}")

# the C ABI alone, on preallocated buffers
units = int(lib.gsr_pose_loss_units(len(lengths), (ctypes.c_int32 * len(packed.offsets))(*packed.offsets)))
host = (ctypes.c_int32 * len(packed.offsets))(*packed.offsets)
f32 = dict(dtype=torch.float32, device=dev)
part_f, part_b, lists, out = torch.empty((units, 4), **f32), torch.empty((units, 12), **f32), torch.empty((len(lengths), 4), **f32), torch.empty(4, **f32)
d_xyz, d_depth, d_poses, up = torch.empty_like(xyz), torch.empty((B, V, H, W), **f32), torch.empty_like(poses), torch.ones(1, **f32)
head = (B, V, H, W, V * (V - 1) // 2, xyz.data_ptr(), depth.data_ptr(), poses.data_ptr(), intr.data_ptr(), packed.ids_i.data_ptr(),
        packed.ids_j.data_ptr(), packed.weights.data_ptr(), packed.conf.data_ptr(), host, packed.offsets_device.data_ptr(), W2D, W3D)
stream = _stream_ptr(dev)


def c_fwd():
    assert lib.gsr_pose_loss(*head, part_f.data_ptr(), lists.data_ptr(), out.data_ptr(), stream) == 0


def c_bwd():
    assert lib.gsr_pose_loss_backward(*head, lists.data_ptr(), up.data_ptr(), d_xyz.data_ptr(), d_depth.data_ptr(), d_poses.data_ptr(),
                                      part_b.data_ptr(), stream) == 0


def launches(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def timed(fn, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / count


legs = {"C ABI  gsr_pose_loss (2 launches)": (c_fwd, reps), "C ABI  gsr_pose_loss_backward (2 memsets + 2 launches)": (c_bwd, reps),
        "HIP    pose_loss forward": (hip_fwd, reps), "HIP    pose_loss forward + backward": (hip_fwd_bwd, reps),
        "HIP    pack + forward + backward": (hip_pack_fwd_bwd, reps),
        "torch  loop form forward": (loop_fwd, loop_reps), "torch  loop form forward + backward": (loop_fwd_bwd, loop_reps)}
for name, (fn, _) in legs.items():
    try:
        print(f"{name:55s} {launches(fn):5d} device activities (kernels, memsets, copies) per call")
    except Exception as e:  # the count is a by-product: the timing below does not depend on it
        print(f"{name:55s} launch count unavailable: {type(e).__name__}: {e}")
for fn, count in legs.values():
    timed(fn, max(3, count // 10))
times = {name: [] for name in legs}
for _ in range(rounds):
    for name, (fn, count) in legs.items():
        times[name].append(timed(fn, count))
for name, ts in times.items():
    print(f"{name:55s} median {sorted(ts)[len(ts) // 2]:9.1f} us   min {min(ts):9.1f}   max {max(ts):9.1f}   ({rounds} x {legs[name][1]} calls)")
