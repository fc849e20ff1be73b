"""Generates tests/golden/cost_volume_fixtures.npz by IMPORTING the reference's cost-volume functions
(src/model/encoder/costvolume/depth_predictor_multiview.py: `prepare_feat_proj_data_lists` and `warp_with_pose_depth_candidates`) on
the CPU, with a stub for the one module that file imports and these functions do not need (`.ldm_unet.unet`), and evaluating the
correlation of `DepthPredictorMultiView.forward` (lines 323-343: per other view the product with the row's own features summed over
c and divided by sqrt(c), then the mean over the other views) on what they return.  Per case: the seeded inputs of
tests/cost_volume_ref.build_case, the reference's float32 volume and autograd's dL/dfeatures for the seeded cotangent.

    python tests/golden/make_cost_volume_fixtures.py <path of a PF3plat checkout>
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
OUT = os.path.join(HERE, "cost_volume_fixtures.npz")
# name: (seed, b, v, c, h, w, D, spread)
CASES = {"v2": (11, 2, 2, 8, 6, 9, 5, 0.02), "v3": (3, 1, 3, 5, 7, 4, 6, 0.1)}


def import_reference(root):
    for name, path in [("src", "src"), ("src.model", "src/model"), ("src.model.encoder", "src/model/encoder"),
                       ("src.model.encoder.costvolume", "src/model/encoder/costvolume"),
                       ("src.model.encoder.costvolume.ldm_unet", "src/model/encoder/costvolume/ldm_unet")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(root, path)]
        sys.modules[name] = m
    unet = types.ModuleType("src.model.encoder.costvolume.ldm_unet.unet")
    unet.UNetModel = object
    sys.modules[unet.__name__] = unet
    return importlib.import_module("src.model.encoder.costvolume.depth_predictor_multiview")


def reference_volume(mod, features, intrinsics, extrinsics, near, far, num):
    c = features.shape[2]
    feats, intr, poses, disp = mod.prepare_feat_proj_data_lists(features, intrinsics, extrinsics, near, far, num_samples=num)
    own = feats[0]
    per_view = []
    for other, pose in zip(feats[1:], poses):
        warped = mod.warp_with_pose_depth_candidates(other, intr, pose, 1.0 / disp.repeat([1, 1, *other.shape[-2:]]), warp_padding_mode="zeros")
        per_view.append((own.unsqueeze(2) * warped).sum(1) / (c ** 0.5))
    return torch.mean(torch.stack(per_view, dim=0), dim=0, keepdim=False)


def main():
    from tests import cost_volume_ref as ref

    mod = import_reference(sys.argv[1])
    out = {}
    for name, (seed, b, v, c, h, w, num, spread) in CASES.items():
        case = ref.build_case(seed, b, v, c, h, w, num, spread)
        f = case["features"].clone().requires_grad_(True)
        cost = reference_volume(mod, f, case["intrinsics"], case["extrinsics"], case["near"], case["far"], num)
        (grad,) = torch.autograd.grad(cost, f, case["cotangent"])
        for key in ("features", "intrinsics", "extrinsics", "near", "far", "cotangent"):
            out[f"{name}.{key}"] = case[key].numpy()
        out[f"{name}.num"] = np.int64(num)
        out[f"{name}.cost"] = cost.detach().numpy()
        out[f"{name}.grad_features"] = grad.numpy()
        print(name, tuple(cost.shape), "zero share", float((cost == 0).double().mean()))
    np.savez_compressed(OUT, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
