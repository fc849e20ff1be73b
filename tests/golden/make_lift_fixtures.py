"""Generates tests/golden/lift_fixtures.npz by IMPORTING the reference's `sample_image_grid`, `unproject` and `get_world_rays`
(src/geometry/projection.py) on the CPU, with the stub `jaxtyping` the other makers use, and evaluating the depth-lift block of
`EncoderCostVolume.forward` (src/model/encoder/encoder_costvolume.py:265, 287-307, 387-392) around them: the lines between those
calls are plain torch calls (two clamps, a bilinear resize, an argmin over |down - hypotheses|, a cross product), written here anew.
Per case: the seeded inputs of tests/lift_ref.build_case, the reference's float32 depth and xyz, the cue's channel per quarter
pixel, the Pluecker map at quarter resolution and autograd's gradients for the seeded cotangents.

    python tests/golden/make_lift_fixtures.py <path of a PF3plat checkout>
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "lift_fixtures.npz")
# name: (seed, b, v, h, w, D)
CASES = {"fixture_a": (21, 2, 2, 8, 12, 128), "fixture_b": (22, 1, 3, 13, 18, 128)}


def import_projection(root):
    jt = types.ModuleType("jaxtyping")

    class _T:
        def __class_getitem__(cls, item):
            return cls

    for n in ("Float", "Bool", "Int64", "Shaped", "Int", "UInt8"):
        setattr(jt, n, _T)
    sys.modules["jaxtyping"] = jt
    for name, path in [("src", "src"), ("src.geometry", "src/geometry")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(root, path)]
        sys.modules[name] = m
    return importlib.import_module("src.geometry.projection")


def reference_block(mod, depth_raw, shift, near, far, intrinsics, c2w, num):
    b, v = near.shape
    h, w = depth_raw.shape[-2:]
    lo, hi = near.reshape(b * v, 1, 1, 1), far.reshape(b * v, 1, 1, 1)
    depth = (depth_raw.clamp(lo, hi) + shift).clamp(lo, hi)
    # the mono cue: hypotheses from the host values of scene 0, view 0 (the reference's .item() calls), float32 linspace
    down = F.interpolate(depth, (h // 4, w // 4), mode="bilinear")
    first, last = (1.0 / far)[0, 0].item(), (1.0 / near)[0, 0].item()
    hyp = (first + torch.linspace(0.0, 1.0, num).unsqueeze(0) * (last - first)).view(1, -1, 1, 1)
    channel = torch.argmin(torch.abs(down - hyp), dim=1)                                   # ((b v), hq, wq)
    channel = channel.reshape(b, v, h // 4, w // 4).transpose(0, 1).reshape(v * b, h // 4, w // 4)
    # the points
    grid, _ = mod.sample_image_grid((h, w))                                                # (h, w, 2)
    coords = grid.reshape(1, h * w, 2).expand(b * v, -1, -1)
    xyz = mod.unproject(coords, depth.reshape(b * v, h * w), intrinsics.reshape(b * v, 1, 3, 3))   # ((b v), hw, 3)
    xyz = xyz.reshape(b, v, h, w, 3).permute(0, 1, 4, 2, 3)
    # the ray map at quarter resolution
    hq, wq = h // 4, w // 4
    grid_q, _ = mod.sample_image_grid((hq, wq))
    origins, directions = mod.get_world_rays(grid_q.reshape(1, 1, hq * wq, 2), c2w.reshape(b, v, 1, 4, 4), intrinsics.reshape(b, v, 1, 3, 3))
    rays = torch.cat((directions, torch.cross(origins, directions, dim=-1)), dim=-1)       # (b, v, hw, 6)
    rays = rays.reshape(b * v, hq, wq, 6).permute(0, 3, 1, 2)
    return depth, xyz, channel, rays


def main():
    from tests import lift_ref as ref

    mod = import_projection(sys.argv[1])
    out = {}
    for name, (seed, b, v, h, w, num) in CASES.items():
        case = ref.build_case(seed, b, v, h, w, num)
        raw, shift, K = (case[k].clone().requires_grad_(True) for k in ("depth_raw", "shift", "intrinsics"))
        depth, xyz, channel, rays = reference_block(mod, raw, shift, case["near"], case["far"], K, case["c2w"], num)
        grads = torch.autograd.grad([depth, xyz], [raw, shift, K], [case["g_depth"], case["g_xyz"]])
        for key in ("depth_raw", "shift", "near", "far", "intrinsics", "c2w", "g_depth", "g_xyz"):
            out[f"{name}.{key}"] = case[key].numpy()
        out[f"{name}.num"] = np.int64(num)
        out[f"{name}.depth"] = depth.detach().numpy()
        out[f"{name}.xyz"] = xyz.detach().numpy()
        out[f"{name}.channel"] = channel.numpy().astype(np.int16)
        out[f"{name}.plucker"] = rays.detach().numpy()
        for key, grad in zip(("d_depth_raw", "d_shift", "d_intrinsics"), grads):
            out[f"{name}.{key}"] = grad.numpy()
        print(name, tuple(xyz.shape), "channels hit", int(channel.unique().numel()))
    np.savez_compressed(OUT, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
