"""The yardstick of the refined-pose tests: the reference's lines after the pose transformer
(src/model/encoder/encoder_costvolume.py:447-450, 460-473 with r6d2mat :189-209 and matrix_to_rotation_6d :223-224, the `.inverse()` of
:492, :530 and src/model/model_wrapper.py:150) and its pose diagnostics (model_wrapper.py:182-190, 306-313; src/flow_util.py:20-32)
restated as torch functions with a dtype switch - float64 is the reference, float32 measures what the reference's own eager arithmetic
loses -, the seeded cases and the error measures.  CPU only."""
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_refine_fixtures.npz")
RECORDS = {"record_a": (2, 2), "record_b": (1, 3)}  # what the reference's own functions computed: tests/golden/make_pose_refine_fixtures.py
CHANNELS = 139  # the pose head's output: 9 pose channels, the feature residual, 2 more
MIN_SIN = 0.5   # build_case: |sin angle(a1, a2)| of every encoded pair
ANGLES = (5.0, 175.0)  # build_case: the relative rotation and the angle between the translation directions, degrees

# What the float32 restatement loses against float64 at worst over CASES and MODES (the measures of `errors_between`; printed by
# tests/test_pose_refine.py::test_floors_are_of_the_size_of_the_worst_float32_loss): the floor of the bars of the GPU tests.  The
# figure depends on the CPU (torch's vectorised sums and LAPACK's LU take another order on another host); each floor is the geometric
# mean of the two hosts' figures, the development machine's and the MI355X host's, which docs/PARITY.md section 19 holds.
FLOOR = {"c2w": 5.9e-8, "w2c": 1.1e-7, "ddelta": 2.3e-7, "dgamma": 1.2e-7, "rotation": 1.5e-7, "translation_angle": 1.8e-7,
         "translation_distance": 8.1e-8}
POSE_KEYS = ("c2w", "w2c", "ddelta", "dgamma")
ERROR_KEYS = ("rotation", "translation_angle", "translation_distance")

# name: (seed, b, v, kind, gamma).  264 poses are past one 256-thread block of the forward; at 520 the backward's stride loop makes a
# third trip, partly empty.
CASES = {
    "b1v1": (1, 1, 1, "plain", 1.0),
    "b1v2": (2, 1, 2, "plain", 1.0),
    "b2v3": (3, 2, 3, "skewed", -0.7),
    "b4v3": (4, 4, 3, "plain", 1.0),
    "b4v3_gamma0": (5, 4, 3, "plain", 0.0),
    "b4v3_skewed": (6, 4, 3, "skewed", 1.0),
    "b2v3_eye0": (7, 2, 3, "eye0", 1.0),
    "b33v8": (8, 33, 8, "plain", -0.7),
    "b129v2": (9, 129, 2, "skewed", 1.0),
    "b65v8": (10, 65, 8, "plain", 1.0),
    "b65v8_skewed": (11, 65, 8, "skewed", -0.7),
}
MODES = ("both", "c2w", "w2c")  # which cotangents the backward gets


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def matrix_to_rotation_6d(pose_mtx):
    return pose_mtx[..., :2, :].clone().reshape(*pose_mtx.size()[:-2], 6)


def r6d2mat(d6):
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = F.normalize(b2, dim=-1)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-2)


def pose_encoding(init_pose):
    return torch.cat([matrix_to_rotation_6d(init_pose[:, :, :3, :3]), init_pose[:, :, :3, 3]], dim=-1)


def refine(sync_abspose, delta, gamma, dtype=torch.float64, rigid=False):
    """(b, v, 4, 4), (b, v, >= 9), gamma -> (c2w, w2c) in `dtype`: lines 447-450 and 465-473, then the reference's `.inverse()` - or,
    with `rigid`, [R^T | -R^T t], the form the kernel takes."""
    init_pose, delta = sync_abspose.to(dtype), delta.to(dtype)
    gamma = gamma.to(dtype) if isinstance(gamma, torch.Tensor) else gamma
    pred_pose_enc = pose_encoding(init_pose)
    pred_pose = pred_pose_enc[:, 1:] + delta[..., :9][:, 1:] * gamma
    pred_concat_pose = torch.cat([pred_pose_enc[:, :1], pred_pose], dim=1)
    rot6d = r6d2mat(pred_concat_pose[:, :, :6])
    trans3d = pred_concat_pose[:, :, 6:]
    Rt = torch.cat([rot6d, trans3d[..., None]], dim=-1)
    pad = torch.zeros_like(Rt[..., 2:3, :])
    pad[..., -1] = 1.0
    c2w = torch.cat((Rt, pad), dim=-2)
    if not rigid:
        return c2w, c2w.inverse()
    Rinv = rot6d.transpose(-1, -2)
    w2c = torch.cat((torch.cat([Rinv, -(Rinv @ trans3d[..., None])], dim=-1), pad), dim=-2)
    return c2w, w2c


def pose_errors(c2w, extrinsics, dtype=torch.float64):
    """Per scene (b,): the geodesic angle (radians), the angle between the translation directions (degrees) and the distance of the
    translations of c2w[:, -1] against extrinsics[:, -1]^-1 extrinsics[:, 0]."""
    c2w, extrinsics = c2w.to(dtype), extrinsics.to(dtype)
    gt_relpose = torch.matmul(extrinsics[:, -1].inverse(), extrinsics[:, 0])
    norm_pred = c2w[:, -1, :3, 3] / torch.linalg.norm(c2w[:, -1, :3, 3], dim=-1).unsqueeze(-1)
    norm_gt = gt_relpose[:, :3, 3] / torch.linalg.norm(gt_relpose[:, :3, 3], dim=-1).unsqueeze(-1)
    angle = torch.arccos(torch.clip((norm_pred * norm_gt).sum(-1), -1.0, 1.0)) * 180 / np.pi
    m = torch.bmm(c2w[:, -1, :3, :3], gt_relpose[:, :3, :3].transpose(1, 2))
    cos = (m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2] - 1) / 2
    theta = torch.acos(torch.clip(cos, -1.0, 1.0))
    distance = torch.linalg.norm(c2w[:, -1, :3, 3] - gt_relpose[:, :3, 3], dim=-1)
    return {"rotation": theta, "translation_angle": angle, "translation_distance": distance}


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def _rotations(g, *lead):
    q = torch.randn(*lead, 4, generator=g, dtype=torch.float64)
    w, x, y, z = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)), -1).reshape(*lead, 3, 3)


def _axis_angle(axis, angle):
    axis = axis / axis.norm(dim=-1, keepdim=True)
    x, y, z = axis.unbind(-1)
    zero = torch.zeros_like(x)
    K = torch.stack((zero, -z, y, z, zero, -x, -y, x, zero), -1).reshape(*axis.shape[:-1], 3, 3)
    s, c = torch.sin(angle)[..., None, None], torch.cos(angle)[..., None, None]
    return torch.eye(3, dtype=axis.dtype) + s * K + (1 - c) * (K @ K)


def _rigid(R, t):
    P = torch.zeros(*R.shape[:-2], 4, 4, dtype=R.dtype)
    P[..., :3, :3], P[..., :3, 3], P[..., 3, 3] = R, t, 1.0
    return P


def min_sin(sync, delta, gamma):
    """The smallest |sin angle(a1, a2)| over the encoded pairs, float64."""
    enc = pose_encoding(sync.double())
    enc = torch.cat([enc[:, :1], enc[:, 1:] + delta.double()[..., :9][:, 1:] * gamma], dim=1)
    a1, a2 = enc[..., :3], enc[..., 3:6]
    return float((torch.cross(a1, a2, dim=-1).norm(dim=-1) / (a1.norm(dim=-1) * a2.norm(dim=-1))).min())


def build_case(seed, b, v, kind, gamma=1.0):
    """sync (b, v, 4, 4), full (b, v, 139) - delta is full[..., :9]; the other channels hold values of the scale 1e3 that nothing may
    read -, the cotangents of c2w and w2c, and ground-truth extrinsics whose relative pose lies 5 to 175 degrees from the refined
    last view in rotation and in the direction of the translation (v >= 2).  float32, seeded.  kind: "plain" rotations of unit
    quaternions; "skewed" rows that are not orthonormal (a1 of norm 3, a2 + 0.3 a1); "eye0" the identity as view 0."""
    assert kind in ("plain", "skewed", "eye0"), kind
    gamma = float(torch.tensor(gamma, dtype=torch.float32))  # (the value a float32 parameter holds)
    g = torch.Generator().manual_seed(int(seed))
    R = _rotations(g, b, v)
    t = torch.rand(b, v, 3, generator=g, dtype=torch.float64) * 4.0 - 2.0
    if kind == "skewed":
        R = R.clone()
        R[..., 0, :] = 3.0 * R[..., 0, :]
        R[..., 1, :] = R[..., 1, :] + 0.3 * R[..., 0, :]
    sync = _rigid(R, t)
    if kind == "eye0":
        sync[:, 0] = torch.eye(4, dtype=torch.float64)
    full = 1e3 * torch.randn(b, v, CHANNELS, generator=g, dtype=torch.float64)
    full[..., :9] = 0.05 * torch.randn(b, v, 9, generator=g, dtype=torch.float64)
    cot_c2w, cot_w2c = (torch.randn(b, v, 4, 4, generator=g, dtype=torch.float64) for _ in range(2))
    f = lambda x: x.to(torch.float32).contiguous()
    case = {"sync": f(sync), "full": f(full), "gamma": gamma, "cot_c2w": f(cot_c2w), "cot_w2c": f(cot_w2c)}
    case["min_sin"] = min_sin(case["sync"], case["full"], gamma)
    assert case["min_sin"] >= MIN_SIN, (seed, b, v, kind, case["min_sin"])
    # ground truth: gt_rel = the refined last pose turned by 20 .. 160 degrees, its translation turned likewise and rescaled
    with torch.no_grad():
        pred = refine(case["sync"], case["full"], gamma)[0][:, -1]
    turn = _axis_angle(torch.randn(b, 3, generator=g, dtype=torch.float64), math.radians(20.0) + math.radians(140.0) * torch.rand(b, generator=g, dtype=torch.float64))
    tp = pred[:, :3, 3]
    side = torch.cross(tp, torch.randn(b, 3, generator=g, dtype=torch.float64), dim=-1)
    swing = _axis_angle(side, math.radians(20.0) + math.radians(140.0) * torch.rand(b, generator=g, dtype=torch.float64))
    gt_rel = _rigid(turn @ pred[:, :3, :3], (swing @ tp[..., None])[..., 0] * (0.5 + torch.rand(b, 1, generator=g, dtype=torch.float64)))
    E0 = _rigid(_rotations(g, b), torch.rand(b, 3, generator=g, dtype=torch.float64) * 4.0 - 2.0)
    ext = _rigid(_rotations(g, b, v), torch.rand(b, v, 3, generator=g, dtype=torch.float64) * 4.0 - 2.0)
    ext[:, 0] = E0
    if v >= 2:
        ext[:, -1] = E0 @ torch.linalg.inv(gt_rel)  # E[-1]^-1 E[0] = gt_rel
    case["extrinsics"] = f(ext)
    if v >= 2:
        with torch.no_grad():
            e = pose_errors(pred[:, None], case["extrinsics"])
        case["angles"] = (float(torch.rad2deg(e["rotation"]).min()), float(torch.rad2deg(e["rotation"]).max()),
                          float(e["translation_angle"].min()), float(e["translation_angle"].max()))
        assert ANGLES[0] <= min(case["angles"]) and max(case["angles"]) <= ANGLES[1], (seed, b, v, kind, case["angles"])
    return case


@functools.lru_cache(maxsize=None)
def record(name):
    with np.load(FIXTURES) as f:
        rec = {key[len(name) + 1:]: torch.from_numpy(f[key]) for key in f.files if key.startswith(name + ".")}
    rec["gamma"] = float(rec["gamma"])
    return rec


@functools.lru_cache(maxsize=None)
def case_of(name):
    return record(name) if name in RECORDS else build_case(*CASES[name])


def cotangents(case, mode):
    return (case["cot_c2w"] if mode in ("both", "c2w") else None, case["cot_w2c"] if mode in ("both", "w2c") else None)


def evaluate(fn, case, mode="both", device=None, strided=True, dtype=torch.float32):
    """c2w, w2c of fn(sync, delta, gamma) with delta = full[..., :9] (or its contiguous copy) and gamma a 0-dim tensor; ddelta (b, v, 9)
    and dgamma at the case's cotangents, the leaves in `dtype` (a gradient comes back in its leaf's)."""
    mv = (lambda x: x.clone()) if device is None else (lambda x: x.to(device))
    sync, full = mv(case["sync"]), mv(case["full"]).to(dtype).requires_grad_(True)
    gamma = torch.tensor(case["gamma"], dtype=dtype, device=sync.device).requires_grad_(True)
    delta = full[..., :9] if strided else full[..., :9].contiguous()
    c2w, w2c = fn(sync, delta, gamma)
    out = {"c2w": c2w.detach(), "w2c": w2c.detach()}
    g1, g2 = cotangents(case, mode)
    loss = sum((o * g.to(o.device, o.dtype)).sum() for o, g in ((c2w, g1), (w2c, g2)) if g is not None)
    if c2w.shape[1] == 1 and not loss.requires_grad:  # (one view: nothing is refined and torch's graph is empty)
        out["dfull"], out["dgamma"] = torch.zeros_like(full), torch.zeros_like(gamma)
    else:
        out["dfull"], out["dgamma"] = torch.autograd.grad(loss, (full, gamma), allow_unused=True)
        out["dfull"] = torch.zeros_like(full) if out["dfull"] is None else out["dfull"]
        out["dgamma"] = torch.zeros_like(gamma) if out["dgamma"] is None else out["dgamma"]
    out["ddelta"] = out["dfull"][..., :9]
    return out


@functools.lru_cache(maxsize=None)
def restatement(name, dtype=torch.float64, mode="both"):
    """The reference's lines on the CPU in `dtype` with `.inverse()`, computed once per case and shared (do not write into it); the
    three pose errors of its c2w against the case's extrinsics with it."""
    case = case_of(name)
    out = evaluate(lambda s, d, g: refine(s, d, g, dtype), case, mode, dtype=dtype)
    if case["sync"].shape[1] >= 2:
        with torch.no_grad():
            out.update(pose_errors(out["c2w"], case["extrinsics"], dtype))
    if dtype == torch.float64:  # what dgamma is a sum of: dL_denc, the gradient of an additive probe on the encoding
        delta = case["full"].double()[..., :9]
        probe = torch.zeros_like(delta).requires_grad_(True)
        c2w, w2c = refine(case["sync"], delta * case["gamma"] + probe, 1.0)
        g1, g2 = cotangents(case, mode)
        loss = sum((o * g.double()).sum() for o, g in ((c2w, g1), (w2c, g2)) if g is not None)
        denc = torch.autograd.grad(loss, probe)[0] if loss.requires_grad else torch.zeros_like(probe)
        out["dgamma_scale"] = float((delta[:, 1:] * denc[:, 1:]).abs().sum())
    return out


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def errors_between(got, r64, keys):
    """Per quantity the project's rel-L2 against float64; dgamma - one number, a sum of terms of both signs - against the sum of the
    terms' magnitudes, the scale a sum's rounding error has."""
    out = {}
    for key in keys:
        if key == "dgamma":
            out[key] = abs(float(got[key]) - float(r64[key])) / max(r64["dgamma_scale"], 1e-300)
        else:
            out[key] = rel_l2(got[key], r64[key])
    return out


def keys_of(name):
    """The quantities a case is judged on: no gradient where nothing is refined (one view), no ddelta at gamma = 0 (exactly zero,
    checked as such), no pose errors for one view (gt_rel is the identity: a zero translation)."""
    b, v = case_of(name)["sync"].shape[:2]
    keys = ["c2w", "w2c"]
    if v >= 2:
        keys += (["ddelta"] if case_of(name)["gamma"] != 0.0 else []) + ["dgamma"]
    return tuple(keys)


def float32_loss(name, mode="both"):
    r64, r32 = restatement(name, torch.float64, mode), restatement(name, torch.float32, mode)
    keys = keys_of(name) + (ERROR_KEYS if mode == "both" and "rotation" in r64 else ())
    return errors_between(r32, r64, keys)


def bars(name, mode="both"):
    """Per quantity: max(FLOOR, 4 x what the float32 restatement loses on this case)."""
    return {key: max(FLOOR[key], 4.0 * lost) for key, lost in float32_loss(name, mode).items()}
