"""Generates tests/golden/pose_sync_fixtures.npz by IMPORTING the reference's `camera_synchronization` (src/flow_util.py:623-743) on the
CPU, with stub modules for what flow_util imports and the function does not use (cv2, open3d, pytorch3d.ops): seeded pairwise poses
and confidences for v = 2, 3, 4 and b = 1, 2, one scene whose far pair's mean score lies below confidence_min, and one scene whose
confidences are all zero - recorded with b = 1, where the reference's batch-wide fallback to camera_chaining is the per-scene one;
then v5_b2, v6_b1, v8_b1, v8_b2 and zero_v5 (five views, every confidence 0).
The confidences go through the encoder's own lines (src/model/encoder/encoder_costvolume.py:370-373) first.

    python tests/golden/make_pose_sync_fixtures.py <path of a PF3plat checkout>
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
OUT = os.path.join(HERE, "pose_sync_fixtures.npz")
CONFIDENCE_MIN = 0.5


def import_flow_util(root):
    for name in ("cv2", "open3d", "pytorch3d", "pytorch3d.ops"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["pytorch3d.ops"].corresponding_points_alignment = None
    m = types.ModuleType("src")
    m.__path__ = [os.path.join(root, "src")]
    sys.modules["src"] = m
    return importlib.import_module("src.flow_util")


def scene_inputs(rng, v, b):
    """Pairwise poses (b, P, 4, 4) float32 - relative poses of v random cameras, each disturbed a little, so that the pairs disagree
    as estimates do - and mean scores (P b,) in list order."""
    from tests import pnp_ref

    pairs = pnp_ref.pairs_of(v)
    Ps = np.zeros((b, len(pairs), 4, 4), dtype=np.float32)
    for s in range(b):
        cams = []
        for _ in range(v):
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = pnp_ref.rodrigues(rng.normal(size=3) * 0.3), rng.normal(size=3) * 0.5
            cams.append(T)
        for p, (i, j) in enumerate(pairs):
            noise = np.eye(4)
            noise[:3, :3], noise[:3, 3] = pnp_ref.rodrigues(rng.normal(size=3) * 0.02), rng.normal(size=3) * 0.03
            Ps[s, p] = (noise @ cams[j] @ np.linalg.inv(cams[i])).astype(np.float32)
    means = rng.uniform(0.55, 0.95, len(pairs) * b).astype(np.float32)
    return Ps, means


def run_reference(fu, Ps, means, v):
    b = Ps.shape[0]
    from tests import pnp_ref

    pairs = pnp_ref.pairs_of(v)
    poses, conf, listed = {}, {}, []
    for p, (i, j) in enumerate(pairs):
        conf_ij = torch.stack([torch.tensor(means[p * b + s]) for s in range(b)])
        if abs(i - j) > 1:
            conf_ij = (conf_ij - CONFIDENCE_MIN).relu()
            conf_ij = conf_ij / (1 - CONFIDENCE_MIN)
        conf[(i, j)] = conf_ij
        poses[(i, j)] = torch.from_numpy(Ps[:, p].copy())
        listed.append(conf_ij)
    out = fu.camera_synchronization(poses, conf, v)
    assert out.dtype == torch.float32 and tuple(out.shape) == (b, v, 4, 4)
    return out.numpy(), torch.cat(listed).numpy()


def main():
    fu = import_flow_util(sys.argv[1])
    rng = np.random.default_rng(2024)
    out, names = {}, []

    def record(name, Ps, means, v):
        absolute, conf = run_reference(fu, Ps, means, v)
        out[name + "/pairwise"], out[name + "/means"], out[name + "/confidence"], out[name + "/absolute"] = Ps, means, conf, absolute
        out[name + "/views"] = np.array(v)
        names.append(name)

    for v in (2, 3, 4):
        for b in (1, 2):
            record(f"v{v}_b{b}", *scene_inputs(rng, v, b), v)
    Ps, means = scene_inputs(rng, 3, 1)
    means[1] = 0.3  # pair (0, 2): below confidence_min, confidence 0
    record("far_low", Ps, means, 3)
    Ps, means = scene_inputs(rng, 3, 1)
    means[:] = 0.0  # every confidence 0: the mass is 0 and the reference chains
    record("zero", Ps, means, 3)
    # Appended after the records above, which stay bit for bit what they were (the generator's draws continue): 5, 6 and 8 views - a
    # matrix of up to 32 x 32 - and five views with every confidence 0 (the fallback's chaining stride past four views).
    for v, b in ((5, 2), (6, 1), (8, 1), (8, 2)):
        record(f"v{v}_b{b}", *scene_inputs(rng, v, b), v)
    Ps, means = scene_inputs(rng, 5, 1)
    means[:] = 0.0
    record("zero_v5", Ps, means, 5)
    out["names"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
