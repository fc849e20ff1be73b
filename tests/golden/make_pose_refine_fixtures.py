"""Generates tests/golden/pose_refine_fixtures.npz by EVALUATING the reference's own functions on the CPU: `r6d2mat` and
`matrix_to_rotation_6d` (methods of the encoder, src/model/encoder/encoder_costvolume.py:189-209, 223-224) and
`compute_geodesic_distance_from_two_matrices` (src/flow_util.py:20-32).  Neither module can be imported here (cv2, the networks), so the
three function definitions are taken out of the two files with `ast` at generation time and executed in a namespace that holds
`torch` and `F`; nothing of their text is written anywhere.  The lines between them - :448-450, :465-473, the `.inverse()` of :492 and
model_wrapper.py:182-186, 313 - are plain torch and are written anew below.  Per record: the inputs (sync, delta, gamma, the two
cotangents, the ground-truth extrinsics), c2w, w2c, autograd's gradients for the cotangents and the three reference scalars, float32.

    python tests/golden/make_pose_refine_fixtures.py <path of a PF3plat checkout>
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "pose_refine_fixtures.npz")
# name: (seed, b, v, kind, gamma)
RECORDS = {"record_a": (101, 2, 2, "plain", 0.8), "record_b": (102, 1, 3, "skewed", -0.6)}


def reference_functions(root):
    """{name: function} of the three definitions, compiled from the reference's files as they stand."""
    wanted = {"src/model/encoder/encoder_costvolume.py": ("r6d2mat", "matrix_to_rotation_6d"),
              "src/flow_util.py": ("compute_geodesic_distance_from_two_matrices",)}
    space = {"torch": torch, "F": F}
    for path, names in wanted.items():
        with open(os.path.join(root, path)) as f:
            tree = ast.parse(f.read())
        found = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name in names]
        assert sorted(n.name for n in found) == sorted(names), (path, [n.name for n in found])
        exec(compile(ast.Module(body=found, type_ignores=[]), path, "exec"), space)
    return space


def run_record(fns, seed, b, v, kind, gamma):
    from tests import pose_refine_ref as ref

    case = ref.build_case(seed, b, v, kind, gamma)
    print(f"({b}, {v}) {kind}: smallest |sin angle(a1, a2)| {case['min_sin']:.4f}; rotation / translation angles {case['angles']}")
    init_pose = case["sync"]
    delta = case["full"][..., :9].contiguous().requires_grad_(True)
    g = torch.tensor(gamma, dtype=torch.float32, requires_grad=True)
    raw_rot = fns["matrix_to_rotation_6d"](None, init_pose[:, :, :3, :3])
    raw_trans = init_pose[:, :, :3, 3]
    pred_pose_enc = torch.cat([raw_rot, raw_trans], dim=-1)
    pred_pose = pred_pose_enc[:, 1:] + delta[:, 1:] * g
    pred_concat_pose = torch.cat([pred_pose_enc[:, :1], pred_pose], dim=1)
    rot6d = fns["r6d2mat"](None, pred_concat_pose[:, :, :6])
    trans3d = pred_concat_pose[:, :, 6:]
    Rt = torch.cat([rot6d, trans3d[..., None]], dim=-1)
    pad = torch.zeros_like(Rt[..., 2:3, :])
    pad[..., -1] = 1.0
    c2w = torch.cat((Rt, pad), dim=-2)
    w2c = c2w.inverse()
    ddelta, dgamma = torch.autograd.grad((c2w * case["cot_c2w"]).sum() + (w2c * case["cot_w2c"]).sum(), (delta, g))
    ext = case["extrinsics"]
    with torch.no_grad():
        gt_relpose = torch.matmul(ext[:, -1].inverse(), ext[:, 0])
        norm_pred = c2w[:, -1, :3, 3] / torch.linalg.norm(c2w[:, -1, :3, 3], dim=-1).unsqueeze(-1)
        norm_gt = gt_relpose[:, :3, 3] / torch.linalg.norm(gt_relpose[:, :3, 3], dim=-1).unsqueeze(-1)
        angle_degree = torch.arccos(torch.clip(torch.dot(norm_pred[0], norm_gt[0]), -1.0, 1.0)) * 180 / np.pi
        geodesic = fns["compute_geodesic_distance_from_two_matrices"](c2w[:, -1, :3, :3], gt_relpose[:, :3, :3])
        translation = torch.linalg.norm(c2w[:, -1, :3, 3] - gt_relpose[:, :3, 3], dim=-1)
    n = lambda t: t.detach().numpy().astype(np.float32)
    return {"sync": n(init_pose), "full": n(case["full"]), "gamma": np.float32(gamma), "cot_c2w": n(case["cot_c2w"]), "cot_w2c": n(case["cot_w2c"]),
            "extrinsics": n(ext), "pose_enc": n(pred_pose_enc), "c2w": n(c2w), "w2c": n(w2c), "ddelta": n(ddelta), "dgamma": n(dgamma),
            "geodesic": n(geodesic), "angle_degree": n(angle_degree), "translation": n(translation)}


def main():
    fns = reference_functions(sys.argv[1])
    out = {}
    for name, args in RECORDS.items():
        for key, value in run_record(fns, *args).items():
            out[f"{name}.{key}"] = value
    np.savez_compressed(OUT, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
