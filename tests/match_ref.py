"""The yardstick of tests/test_match_assignment.py: the reference's MatchAssignment.forward, sigmoid_log_double_softmax and
filter_matches (src/model/LightGlue/lightglue/lightglue.py:259-312) and its list building (:586-597) restated in torch - float64 the
reference, float32 what the reference itself runs - for equal-length and ragged input, the case table with its seeded generators, and
the bars (docs/PARITY.md section 21).

Cases: list 1's descriptors are, for a share of its keypoints, noisy copies of list 0's under a permutation (planted matches), the
rest noise; final_proj's weight is sharpened so that the softmaxes are not flat.  Indices are judged EXACTLY, which is fair only where
no decision lies within rounding: `conditions` measures, in float64, the smallest top-two gap of a's rows and b's columns and the
smallest distance of a mutual score from the threshold, and the CPU test asserts both >= GAP for every case (seeds chosen so).

GAP: 100 x the largest |float32 restatement - float64 restatement| of max0 (the log of the mutual score, over every row of every
case).  FLOOR: the worst rel-L2 loss of the float32 restatement's matching scores over the cases.  Both measured on the CPU the
fixtures were made on; the CPU test checks their order of magnitude on the machine it runs on."""
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "golden", "match_fixtures.npz")
CAP = 1e-4
MAX0_LOSS = 2.9e-5   # measured: the largest |float32 - float64| of max0 over the cases (2.86e-5, case "e323")
GAP = 100 * MAX0_LOSS
FLOOR = 1.3e-6       # measured: the worst float32 rel-L2 loss of the matching scores over the cases (1.26e-6, case "d5")
THRESHOLD = 0.1
# name: (B, m, n, d, seed) - records of the reference's own classes (tests/golden/make_match_fixtures.py)
RECORDS = {"rec256": (2, 70, 150, 256, 21), "rec64": (1, 45, 33, 64, 22)}
RECORD_SHARPEN = 3.0
# name: (seed, ((m, n) per list), d, kind, threshold); kinds: "planted", "big" (|s| reaches 200), "z40" (logits +-40), "select"
CASES = {
    "n77": (1, ((1, 77),), 32, "planted", THRESHOLD),
    "n1": (2, ((40, 1),), 32, "planted", THRESHOLD),
    "e70": (1203, ((70, 150),), 32, "planted", THRESHOLD),
    "e131": (1604, ((131, 323),), 32, "planted", THRESHOLD),
    "e323": (1105, ((323, 131),), 32, "planted", THRESHOLD),
    "e260": (10406, ((260, 517),), 32, "planted", THRESHOLD),
    "d1": (1807, ((70, 150),), 1, "planted", THRESHOLD),
    "d5": (708, ((70, 150),), 5, "planted", THRESHOLD),
    "d31": (709, ((70, 150),), 31, "planted", THRESHOLD),
    "d64": (410, ((70, 150),), 64, "planted", THRESHOLD),
    "d255": (411, ((70, 150),), 255, "planted", THRESHOLD),
    "d256": (612, ((70, 150),), 256, "planted", THRESHOLD),
    "ragged": (2913, ((70, 150), (0, 33), (1, 77), (45, 0), (131, 323), (40, 1)), 32, "planted", THRESHOLD),
    "big": (114, ((70, 150),), 32, "big", THRESHOLD),
    "z40": (15, ((70, 150),), 32, "z40", THRESHOLD),
    "th0": (16, ((70, 150),), 32, "planted", 0.0),
    "th09": (116, ((70, 150),), 32, "planted", 0.9),
    "select": (17, ((256, 256), (256, 256)), 8, "select", THRESHOLD),
}
SELECT_SCALE = 0.5


def rel_l2(a, b):
    a, b = a.double(), b.double()
    den = float(b.norm())
    return float((a - b).norm()) / den if den > 0 else float((a - b).norm())


# ---- the reference's lines ----------------------------------------------------------------------------------------------------------
def sigmoid_log_double_softmax(sim, z0, z1):
    b, m, n = sim.shape
    certainties = F.logsigmoid(z0) + F.logsigmoid(z1).transpose(1, 2)
    scores0 = F.log_softmax(sim, 2)
    scores1 = F.log_softmax(sim.transpose(-1, -2).contiguous(), 2).transpose(-1, -2)
    scores = sim.new_full((b, m + 1, n + 1), 0)
    scores[:, :m, :n] = scores0 + scores1 + certainties
    scores[:, :-1, -1] = F.logsigmoid(-z0.squeeze(-1))
    scores[:, -1, :-1] = F.logsigmoid(-z1.squeeze(-1))
    return scores


def filter_matches(scores, th):
    max0, max1 = scores[:, :-1, :-1].max(2), scores[:, :-1, :-1].max(1)
    m0, m1 = max0.indices, max1.indices
    indices0 = torch.arange(m0.shape[1])[None]
    indices1 = torch.arange(m1.shape[1])[None]
    mutual0 = indices0 == m1.gather(1, m0)
    mutual1 = indices1 == m0.gather(1, m1)
    max0_exp = max0.values.exp()
    zero = max0_exp.new_tensor(0)
    mscores0 = torch.where(mutual0, max0_exp, zero)
    mscores1 = torch.where(mutual1, mscores0.gather(1, m1), zero)
    valid0 = mutual0 & (mscores0 > th)
    valid1 = mutual1 & valid0.gather(1, m1)
    m0 = torch.where(valid0, m0, -1)
    m1 = torch.where(valid1, m1, -1)
    return m0, m1, mscores0, mscores1, max0.values


def assignment(mdesc0, mdesc1, z0, z1, threshold=THRESHOLD, dtype=torch.float64, scale=None):
    """mdesc0 (B, m, d), mdesc1 (B, n, d) - the outputs of final_proj -, z0 (B, m, 1), z1 (B, n, 1) -> the reference's results in
    `dtype`: matches0 / 1 (int64), matching_scores0 / 1, max0 (the log of the score before the mutual check) and the per-list
    `matches` (k, 2) and `scores` (k,).  `scale`: None is the reference's division of both operands by d ** 0.25; a float multiplies
    the similarity in its place (the select case)."""
    B, m, d = mdesc0.shape
    n = mdesc1.shape[1]
    a0, a1, z0, z1 = (t.to(dtype) for t in (mdesc0, mdesc1, z0.reshape(B, m, 1), z1.reshape(B, n, 1)))
    if m == 0 or n == 0:  # lightglue.py:563-583
        return {"matches0": torch.full((B, m), -1), "matches1": torch.full((B, n), -1), "matching_scores0": torch.zeros(B, m, dtype=dtype),
                "matching_scores1": torch.zeros(B, n, dtype=dtype), "max0": torch.zeros(B, m, dtype=dtype),
                "matches": [torch.empty(0, 2, dtype=torch.int64)] * B, "scores": [torch.empty(0, dtype=dtype)] * B}
    if scale is None:
        sim = torch.einsum("bmd,bnd->bmn", a0 / d ** 0.25, a1 / d ** 0.25)
    else:
        sim = torch.einsum("bmd,bnd->bmn", a0, a1) * scale
    m0, m1, ms0, ms1, max0 = filter_matches(sigmoid_log_double_softmax(sim, z0, z1), threshold)
    matches, scores = [], []
    for k in range(B):
        valid = m0[k] > -1
        matches.append(torch.stack([torch.where(valid)[0], m0[k][valid]], -1))
        scores.append(ms0[k][valid])
    return {"matches0": m0, "matches1": m1, "matching_scores0": ms0, "matching_scores1": ms1, "max0": max0, "matches": matches, "scores": scores}


def gaps(mdesc0, mdesc1, z0, z1, scale=None):
    """In float64, for one list: (the smallest top-two gap over a's rows and b's columns, the mutual scores)."""
    m, d = mdesc0.shape
    n = mdesc1.shape[0]
    a0, a1 = mdesc0.double(), mdesc1.double()
    s = (a0 / d ** 0.25) @ (a1 / d ** 0.25).T if scale is None else (a0 @ a1.T) * scale
    lr, lc = torch.logsumexp(s, 1), torch.logsumexp(s, 0)
    a = 2 * s - lc[None] + F.logsigmoid(z1.double().reshape(1, n))
    b = 2 * s - lr[:, None] + F.logsigmoid(z0.double().reshape(m, 1))
    gap = math.inf
    if n >= 2:
        top = a.topk(2, 1).values
        gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
    if m >= 2:
        top = b.topk(2, 0).values
        gap = min(gap, float((top[0] - top[1]).min()))
    return gap, float(s.abs().max())


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def planted_descriptors(g, m, n, d, share=0.6, noise=0.1):
    """x0 (m, d), x1 (n, d): `share` of the shorter side's keypoints have a partner, a noisy copy, under a random permutation."""
    x0, x1 = torch.randn(m, d, generator=g), torch.randn(n, d, generator=g)
    k = int(share * min(m, n))
    if k == 0 and min(m, n) >= 1:
        k = 1
    i, j = torch.randperm(m, generator=g)[:k], torch.randperm(n, generator=g)[:k]
    x1[j] = x0[i] + noise * torch.randn(k, d, generator=g)
    return x0, x1


def select_permutation(seed, l, n):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed + 1000 + l))


@functools.lru_cache(maxsize=None)
def case_of(name):
    """{"lists": [(mdesc0 (m, d), mdesc1 (n, d), z0 (m,), z1 (n,)) per list], "kpts": [(kpts0 (m, 2), kpts1 (n, 2))], "width", "scale",
    "threshold"}, float32."""
    seed, sizes, d, kind, threshold = CASES[name]
    g = torch.Generator().manual_seed(seed)
    lists, kpts, width = [], [], 97
    if kind == "select":
        # +-8 sign codes of the keypoint index: with scale 0.5 the similarity is 256 at j = pi(i) and at most 192 elsewhere
        for l, (m, n) in enumerate(sizes):
            assert m == n and n <= 2 ** d
            bits = ((torch.arange(n)[:, None] >> torch.arange(d)[None, :]) & 1).float() * 16.0 - 8.0
            perm = select_permutation(seed, l, n)
            z0 = ((torch.arange(m) * 7 + l) % 3 != 0).float() * 16.0 - 8.0
            z1 = ((torch.arange(n) * 5 + l) % 4 != 0).float() * 16.0 - 8.0
            lists.append((bits[perm].contiguous(), bits, z0, z1))
    else:
        sharpen = 4.0 / d ** 0.25 if d < 16 else 3.0
        w = torch.randn(d, d, generator=g) * (sharpen / d ** 0.5)
        bias = 0.1 * torch.randn(d, generator=g)
        for m, n in sizes:
            x0, x1 = planted_descriptors(g, m, n, d)
            a0, a1 = x0 @ w.T + bias, x1 @ w.T + bias
            z0, z1 = 2.0 * torch.randn(m, generator=g) + 1.0, 2.0 * torch.randn(n, generator=g) + 1.0
            if kind == "big":
                a0, a1 = 1.6 * a0, 1.6 * a1
            if kind == "z40":
                z0, z1 = torch.sign(z0) * 40.0, torch.sign(z1) * 40.0
            lists.append((a0.contiguous(), a1.contiguous(), z0, z1))
    for m, n in sizes:  # non-integer keypoints inside a 97 x 61 image
        kpts.append((torch.rand(m, 2, generator=g) * torch.tensor([96.0, 60.0]) + 0.01, torch.rand(n, 2, generator=g) * torch.tensor([96.0, 60.0]) + 0.01))
    return {"lists": lists, "kpts": kpts, "width": width, "scale": SELECT_SCALE if kind == "select" else None, "threshold": threshold}


@functools.lru_cache(maxsize=None)
def restatement(name, dtype=torch.float64):
    """Per list of the case, `assignment` at batch 1 with the batch axis removed."""
    case = case_of(name)
    out = []
    for a0, a1, z0, z1 in case["lists"]:
        r = assignment(a0[None], a1[None], z0[None], z1[None], case["threshold"], dtype, case["scale"])
        out.append({k: v[0] for k, v in r.items()})
    return out


@functools.lru_cache(maxsize=None)
def conditions(name):
    """(smallest top-two gap, smallest |mutual score - threshold|, largest |s|, largest |max0 float32 - float64|) over the case's lists."""
    case, r64, r32 = case_of(name), restatement(name), restatement(name, torch.float32)
    gap, dist, big, loss = math.inf, math.inf, 0.0, 0.0
    for (a0, a1, z0, z1), r, q in zip(case["lists"], r64, r32):
        if a0.shape[0] == 0 or a1.shape[0] == 0:
            continue
        g, s = gaps(a0, a1, z0, z1, case["scale"])
        gap, big = min(gap, g), max(big, s)
        mutual = r["matching_scores0"][r["matching_scores0"] > 0]
        if mutual.numel() and case["threshold"] > 0:
            dist = min(dist, float((mutual - case["threshold"]).abs().min()))
        loss = max(loss, float((q["max0"].double() - r["max0"]).abs().max()))
    return gap, dist, big, loss


def scores_of(lists, key):
    return torch.cat([r[key].double().reshape(-1) for r in lists])


def bars(name):
    r64, r32 = restatement(name), restatement(name, torch.float32)
    return {key: max(FLOOR, 4.0 * rel_l2(scores_of(r32, key), scores_of(r64, key))) for key in ("matching_scores0", "matching_scores1", "scores")}


def packed(name):
    """The case as the packed ragged call takes it: (mdesc0, mdesc1, z0, z1, lengths0, lengths1, kpts0, kpts1)."""
    case = case_of(name)
    cat = lambda k: torch.cat([ls[k] for ls in case["lists"]])
    return (cat(0), cat(1), cat(2), cat(3), [ls[0].shape[0] for ls in case["lists"]], [ls[1].shape[0] for ls in case["lists"]],
            torch.cat([k[0] for k in case["kpts"]]), torch.cat([k[1] for k in case["kpts"]]))


# ---- the records of the reference's own classes -------------------------------------------------------------------------------------
def record_inputs(name):
    """desc0 (B, m, d), desc1 (B, n, d) of a record: seeded here, not stored."""
    B, m, n, d, seed = RECORDS[name]
    g = torch.Generator().manual_seed(seed)
    pairs = [planted_descriptors(g, m, n, d) for _ in range(B)]
    return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])


@functools.lru_cache(maxsize=None)
def record(name):
    with np.load(FIXTURES) as f:
        return {k[len(name) + 1:]: torch.from_numpy(f[k]) for k in f.files if k.startswith(name + ".")}


def state_of(name):
    return {k[len("state."):]: v for k, v in record(name).items() if k.startswith("state.")}


def record_restatement(name, dtype=torch.float64):
    """The two projections in `dtype` with the recorded weights, then `assignment`."""
    st = {k: v.to(dtype) for k, v in state_of(name).items()}
    d0, d1 = (t.to(dtype) for t in record_inputs(name))
    proj = lambda x: x @ st["final_proj.weight"].T + st["final_proj.bias"]
    logit = lambda x: x @ st["matchability.weight"].T + st["matchability.bias"]
    return assignment(proj(d0), proj(d1), logit(d0), logit(d1), THRESHOLD, dtype)


# ---- match lists for a planted pose scene (tests/pnp_ref.PlantedScene) ---------------------------------------------------------------
POSE_D, POSE_EXTRA, POSE_SEED = 64, 7, 31


@functools.lru_cache(maxsize=None)
def pose_case(scene_name="mixed"):
    """Descriptors, logits and keypoints whose assignment gives back the planted scene's match lists: list l's first image holds the
    scene's 2-D points (sub-pixel), its second image the pixels of ids_j (plus a sub-pixel offset) under a permutation and POSE_EXTRA
    keypoints without a partner.  Returns the packed operands of one call and the per-list operands."""
    from tests import pnp_ref, test_coarse_pose as cp

    sc = cp.scene(scene_name)
    g = torch.Generator().manual_seed(POSE_SEED)
    lists, kpts = [], []
    for ls in sc.lists:
        m = ls.ids_i.size
        n = m + POSE_EXTRA if m else 0
        x0 = 1.5 * torch.randn(m, POSE_D, generator=g)
        x1 = 1.5 * torch.randn(n, POSE_D, generator=g)
        perm = torch.randperm(n, generator=g)[:m]
        x1[perm] = x0 + 0.05 * torch.randn(m, POSE_D, generator=g)
        k0 = torch.from_numpy(ls.points_2d.astype(np.float32))
        k1 = torch.rand(n, 2, generator=g) * torch.tensor([pnp_ref.W - 1.0, pnp_ref.H - 1.0])
        ids_j = torch.from_numpy(ls.ids_j)
        k1[perm] = torch.stack([(ids_j % pnp_ref.W).float() + 0.25, (ids_j // pnp_ref.W).float() + 0.5], -1)
        lists.append((x0, x1, 3.0 + torch.rand(m, generator=g), 3.0 + torch.rand(n, generator=g)))
        kpts.append((k0, k1))
    return {"scene": sc, "lists": lists, "kpts": kpts, "width": pnp_ref.W}
