"""Generates tests/golden/pose_loss_fixtures.npz by IMPORTING the reference's `Losspose` (src/loss/loss_pose.py) on the CPU, with stub
modules for what it imports and does not use (jaxtyping, cv2, open3d, pytorch3d.ops, the reference's dataset / model packages):
the seeded inputs of tests/pose_loss_ref.build_scene, the loss value and the gradients torch autograd gives through the
reference's own code for `xyz`, `depth` and the top three rows of `poses`.

    python tests/golden/make_pose_loss_fixtures.py <path of a PF3plat checkout>
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "pose_loss_fixtures.npz")
B, V, H, W = 2, 3, 12, 20
LENGTHS = (0, 1, 7, 64, 65, 130)
KINDS = ("near", "random")
WEIGHT_2D, WEIGHT_3D = 0.3, 1.7


def import_losspose(root):
    jt = types.ModuleType("jaxtyping")

    class _T:
        def __class_getitem__(cls, item):
            return cls

    for n in ("Float", "Bool", "Int64", "Shaped", "Int", "UInt8"):
        setattr(jt, n, _T)
    sys.modules["jaxtyping"] = jt
    for name in ("cv2", "open3d", "pytorch3d", "pytorch3d.ops"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["pytorch3d.ops"].corresponding_points_alignment = None
    for name, path in [("src", "src"), ("src.loss", "src/loss"), ("src.geometry", "src/geometry"), ("src.dataset", "src/dataset"),
                       ("src.model", "src/model"), ("src.model.decoder", "src/model/decoder")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(root, path)]
        sys.modules[name] = m
    for name, attrs in (("src.dataset.types", ("BatchedExample",)), ("src.model.decoder.decoder", ("DecoderOutput",)),
                        ("src.model.types", ("Gaussians",))):
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, object)
        sys.modules[name] = m
    lm = types.ModuleType("src.loss.loss")

    class Loss:
        def __class_getitem__(cls, item):
            return cls

    lm.Loss = Loss
    sys.modules["src.loss.loss"] = lm
    return importlib.import_module("src.loss.loss_pose")


def main():
    from tests import pose_loss_ref

    lp = import_losspose(sys.argv[1])
    sc = pose_loss_ref.build_scene(77, B, V, H, W, LENGTHS, KINDS)
    xyz, depth, top = sc.xyz.clone().requires_grad_(True), sc.depth.clone().requires_grad_(True), sc.poses[:, :, :3].clone().requires_grad_(True)
    poses = torch.cat([top, sc.poses[:, :, 3:]], 2)  # the caller pads the bottom row as a constant
    loss = lp.Losspose()
    loss.cfg = lp.LossposeCfg(WEIGHT_2D, WEIGHT_3D)
    image = torch.zeros(B, V, 3, H, W)
    batch = {"context": {"image": image}, "target": {"image": image, "intrinsics": sc.intrinsics}}
    rel = torch.eye(4).repeat(B, len(sc.corr), 1, 1)  # c2w[0]: read, and what is made of it is never returned
    value = loss.forward(None, batch, None, 0, (rel, poses), (depth,), (sc.corr, None, sc.conf), xyz)
    gx, gd, gp = torch.autograd.grad(value, (xyz, depth, top))
    out = {"xyz": sc.xyz, "depth": sc.depth, "poses": sc.poses, "intrinsics": sc.intrinsics, "value": value.detach(),
           "grad_xyz": gx, "grad_depth": gd, "grad_poses_top": gp, "weights": torch.tensor([WEIGHT_2D, WEIGHT_3D]),
           "offsets": torch.tensor(np.cumsum((0,) + LENGTHS))}
    order = [(p, s) for p in pose_loss_ref.pairs_of(V) for s in range(B)]
    for k, name in enumerate(("ids_i", "ids_j", "scores")):
        out[name] = torch.cat([sc.corr[p][s][k] for p, s in order])
    out["conf"] = torch.stack([sc.conf[p][s] for p, s in order])
    out = {k: v.numpy() for k, v in out.items()}
    np.savez_compressed(OUT, **out)
    print({k: v.shape for k, v in out.items()}, float(out["value"]))


if __name__ == "__main__":
    main()
