"""Float64 numpy references for the coarse-pose chain (pf3plat_amd/pose.py; the definition is stated in include/gsr.h): a builder of
planted PnP scenes, Gauss-Newton to convergence on a given inlier set, and a restatement of the reference's
`camera_synchronization` / `camera_chaining` (src/flow_util.py:341-368, 623-743) that keeps the reference's float32 steps in float32.
No test helper here touches a device."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

H, W, FOCAL = 48, 64, 60.0          # not square: an x / y swap shows
DEPTH_LO, DEPTH_HI = 1.5, 6.0
ROTATION, TRANSLATION = 0.08, 0.25  # radians, scene units
NOISE_PX, OUTLIER_MIN_PX = 1.0, 20.0
THRESHOLD = 5.0


def pairs_of(v):
    return [(a, c) for a in range(v) for c in range(a + 1, v)]


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def project(R, t, cam, X):
    """-> (pixels (n, 2), depths (n,)) of the points X (n, 3) under (R, t) and cam = (fx, fy, cx, cy)."""
    Y = X @ R.T + t
    return np.stack([cam[0] * Y[:, 0] / Y[:, 2] + cam[2], cam[1] * Y[:, 1] / Y[:, 2] + cam[3]], 1), Y[:, 2]


def gauss_newton(R, t, cam, X, u, steps=60):
    """The minimiser of sum |pi(K (R X + t)) - u|^2 over the given matches from the given start: Gauss-Newton with the update
    R <- exp(w) R, t <- t + d until the step vanishes (at most `steps`)."""
    R, t = np.array(R, dtype=np.float64), np.array(t, dtype=np.float64)
    X, u = np.asarray(X, dtype=np.float64), np.asarray(u, dtype=np.float64)
    fx, fy = cam[0], cam[1]
    for _ in range(steps):
        Q = X @ R.T
        Y = Q + t
        iz = 1.0 / Y[:, 2]
        r = np.stack([fx * Y[:, 0] * iz + cam[2] - u[:, 0], fy * Y[:, 1] * iz + cam[3] - u[:, 1]], 1)
        a0 = np.stack([fx * iz, np.zeros_like(iz), -fx * Y[:, 0] * iz * iz], 1)
        a1 = np.stack([np.zeros_like(iz), fy * iz, -fy * Y[:, 1] * iz * iz], 1)
        J = np.zeros((X.shape[0], 2, 6))
        J[:, 0, :3], J[:, 1, :3] = np.cross(Q, a0), np.cross(Q, a1)  # d(a . (w x Q)) / dw = Q x a
        J[:, 0, 3:], J[:, 1, 3:] = a0, a1
        J2, r2 = J.reshape(-1, 6), r.reshape(-1)
        step = np.linalg.solve(J2.T @ J2, -J2.T @ r2)
        R, t = rodrigues(step[:3]) @ R, t + step[3:]
        if np.abs(step).max() < 1e-15:
            break
    return R, t


@dataclass
class PlantedList:
    pair: tuple
    scene: int
    ids_i: np.ndarray      # (n,) int64: the pixel nearest the 2-D point, inside the image
    ids_j: np.ndarray      # (n,) int64
    points_2d: np.ndarray  # (n, 2) float32
    scores: np.ndarray     # (n,) float32
    inlier: np.ndarray     # (n,) bool: the planted mask
    R: np.ndarray = None   # the planted pose, u ~ pi(K (R X + t))
    t: np.ndarray = None


@dataclass
class PlantedScene:
    b: int
    v: int
    xyz: np.ndarray         # (b, v, 3, H, W) float32
    intrinsics: np.ndarray  # (b, v, 3, 3) float32, pixel units
    lists: list = field(default_factory=list)  # in the pack's order: l = pair x b + scene

    def cam(self, ls):
        k = self.intrinsics[ls.scene, ls.pair[0]].astype(np.float64)
        return (k[0, 0], k[1, 1], k[0, 2], k[1, 2])

    def points(self, ls):
        return self.xyz[ls.scene, ls.pair[1]].reshape(3, -1)[:, ls.ids_j].T.astype(np.float64)

    def optimum(self, ls):
        """The float64 optimum over the planted inliers, started at the planted pose."""
        m = ls.inlier
        return gauss_newton(ls.R, ls.t, self.cam(ls), self.points(ls)[m], ls.points_2d[m].astype(np.float64))


def build_scene(seed, b, v, specs, behind=(), focal=None):
    """specs: per list, in the pack's order, (n, inlier share, noisy) - share 1 and noisy False: exact matches.  Lists named in
    `behind` have every point behind the camera (the planted pose turns the camera away).  Each view's points are the unprojection
    of a random depth map in [1.5, 6]; a list's 3-D points are those at its ids_j, its planted pose a rotation of about 0.08 rad
    and a translation of about 0.25; inliers carry uniform noise in [-1, 1] px per axis, an outlier's 2-D point is redrawn until
    it lies >= 20 px from its true projection.  The first two non-trivial lists contain ids 0 and H W - 1.  `focal`: (fx, fy), or
    an array that broadcasts to (b, v, 2) for focal lengths per view, in place of FOCAL for both; nothing is drawn for it, and None
    leaves every scene as it was."""
    rng = np.random.default_rng(seed)
    pairs = pairs_of(v)
    assert len(specs) == len(pairs) * b
    K = np.array([[FOCAL, 0, (W - 1) / 2], [0, FOCAL, (H - 1) / 2], [0, 0, 1]], dtype=np.float32)
    intrinsics = np.tile(K, (b, v, 1, 1))
    if focal is not None:
        f = np.broadcast_to(np.asarray(focal, dtype=np.float32), (b, v, 2))
        intrinsics[..., 0, 0], intrinsics[..., 1, 1] = f[..., 0], f[..., 1]
    intrinsics[..., 0, 2] += rng.uniform(-1, 1, (b, v)).astype(np.float32)
    intrinsics[..., 1, 2] += rng.uniform(-1, 1, (b, v)).astype(np.float32)
    ys, xs = np.mgrid[0:H, 0:W]
    xyz = np.zeros((b, v, 3, H, W), dtype=np.float32)
    for s in range(b):
        for j in range(v):
            k = intrinsics[s, j].astype(np.float64)
            d = rng.uniform(DEPTH_LO, DEPTH_HI, (H, W))
            xyz[s, j] = np.stack([(xs - k[0, 2]) / k[0, 0] * d, (ys - k[1, 2]) / k[1, 1] * d, d]).astype(np.float32)
    scene = PlantedScene(b, v, xyz, intrinsics)
    corners = 0
    for l, (n, share, noisy) in enumerate(specs):
        pair, s = pairs[l // b], l % b
        axis = rng.normal(size=3)
        R = rodrigues(axis / np.linalg.norm(axis) * ROTATION)
        t = rng.normal(size=3)
        t = t / np.linalg.norm(t) * TRANSLATION
        if l in behind:
            R = np.diag([-1.0, 1.0, -1.0]) @ R  # (half a turn about y: depths of about -6 .. -1.5)
        k = intrinsics[s, pair[0]].astype(np.float64)
        cam = (k[0, 0], k[1, 1], k[0, 2], k[1, 2])
        allX = xyz[s, pair[1]].reshape(3, -1).T.astype(np.float64)
        uv, _ = project(R, t, cam, allX)
        inside = (uv[:, 0] >= 1.5) & (uv[:, 0] <= W - 2.5) & (uv[:, 1] >= 1.5) & (uv[:, 1] <= H - 2.5)
        pool = np.flatnonzero(inside) if l not in behind else np.arange(H * W)
        ids_j = rng.choice(pool, size=n, replace=n > pool.size) if n else np.zeros(0, dtype=np.int64)
        n_in = int(np.ceil(n * share))
        inlier = np.zeros(n, dtype=bool)
        inlier[rng.permutation(n)[:n_in]] = True
        corner = None
        if n >= 8 and corners < 2 and (~inlier).sum() >= 2:  # ids 0 and H W - 1, in both views, as two outliers
            corner = np.flatnonzero(~inlier)[:2]
            ids_j[corner[0]], ids_j[corner[1]] = 0, H * W - 1
            corners += 1
        true_uv = uv[ids_j]
        pts = true_uv.copy()
        if noisy:
            pts[inlier] += rng.uniform(-NOISE_PX, NOISE_PX, (n_in, 2))
        for m in np.flatnonzero(~inlier):
            while True:
                cand = rng.uniform([0, 0], [W - 1, H - 1])
                if np.linalg.norm(cand - true_uv[m]) >= OUTLIER_MIN_PX:
                    break
            pts[m] = cand
        if corner is not None:
            for m, c in zip(corner, ((W - 1.0, H - 1.0), (0.0, 0.0))):
                assert np.linalg.norm(np.array(c) - true_uv[m]) >= OUTLIER_MIN_PX
                pts[m] = c
        px = np.clip(np.rint(pts[:, 0]), 0, W - 1).astype(np.int64)
        py = np.clip(np.rint(pts[:, 1]), 0, H - 1).astype(np.int64)
        scores = rng.uniform(0.2, 1.0, n).astype(np.float32)
        scene.lists.append(PlantedList(pair, s, py * W + px, ids_j.astype(np.int64), pts.astype(np.float32), scores, inlier, R, t))
    return scene


def repeated_id_list(scene, l, n, pixel):
    """Replace list l by n copies of one match (a degenerate list: no three distinct points)."""
    ls = scene.lists[l]
    scene.lists[l] = PlantedList(ls.pair, ls.scene, np.full(n, pixel, dtype=np.int64), np.full(n, pixel, dtype=np.int64),
                                 np.tile(np.array([[pixel % W, pixel // W]], dtype=np.float32), (n, 1)),
                                 np.full(n, 0.7, dtype=np.float32), np.zeros(n, dtype=bool), ls.R, ls.t)


def expected_confidence(scene, confidence_min=0.5):
    """The lists' confidences as include/gsr.h defines them: the mean score, 0 for an empty list, the relu for far pairs (float32)."""
    out = []
    for ls in scene.lists:
        c = np.float32(ls.scores.astype(np.float64).mean()) if ls.scores.size else np.float32(0)
        if ls.pair[1] - ls.pair[0] > 1:
            c = np.float32(max(np.float32(c - np.float32(confidence_min)), np.float32(0))) / np.float32(np.float32(1) - np.float32(confidence_min))
        out.append(c)
    return np.array(out, dtype=np.float32)


def ulps(got, want):
    """The largest difference of two float32 matrices in float32 ulps of the larger one's largest entry, per matrix."""
    scale = np.abs(want).reshape(*want.shape[:-2], -1).max(-1)
    ulp = np.spacing(scale.astype(np.float32)).astype(np.float64)
    return (np.abs(got.astype(np.float64) - want.astype(np.float64)).reshape(*want.shape[:-2], -1).max(-1) / ulp).max()


# ------------------------------------------------------------------------------------------------------------------------
# camera_synchronization restated
# ------------------------------------------------------------------------------------------------------------------------
def _se3_inverse_f32(P):
    R_inv = P[:3, :3].T
    t_inv = np.zeros(3, dtype=np.float32)
    neg = np.float32(-1) * R_inv
    for r in range(3):
        acc = np.float32(neg[r, 0] * P[0, 3])
        acc = np.float32(acc + np.float32(neg[r, 1] * P[1, 3]))
        acc = np.float32(acc + np.float32(neg[r, 2] * P[2, 3]))
        t_inv[r] = acc
    out = np.zeros((4, 4), dtype=np.float32)
    out[:3, :3], out[:3, 3], out[3] = R_inv, t_inv, P[3]
    return out


def camera_chaining(Ps, v):
    """Ps (P, 4, 4) float32 of one scene -> (v, 4, 4) float32: identity, then P(i, i + 1) @ the pose before it, in float32."""
    pairs = pairs_of(v)
    out = [np.eye(4, dtype=np.float32)]
    for i in range(v - 1):
        P, cur = Ps[pairs.index((i, i + 1))].astype(np.float32), out[-1]
        nxt = np.zeros((4, 4), dtype=np.float32)
        for r in range(4):
            for c in range(4):
                acc = np.float32(P[r, 0] * cur[0, c])
                for k in range(1, 4):
                    acc = np.float32(acc + np.float32(P[r, k] * cur[k, c]))
                nxt[r, c] = acc
        out.append(nxt)
    return np.stack(out)


def camera_synchronization(Ps, confidence, v, squares=10):
    """Ps (P, 4, 4) float32 and confidence (P,) float32 of ONE scene -> (v, 4, 4) float64 (the reference rounds it to float32 at the
    end: compare with `.astype(np.float32)`): the reference at its default arguments, with the fallback to chaining decided for
    this scene alone."""
    Ps, confidence = np.asarray(Ps, dtype=np.float32), np.asarray(confidence, dtype=np.float32)
    if v == 2:
        return camera_chaining(Ps, v).astype(np.float64)
    pairs = pairs_of(v)
    conf = np.zeros((v, v), dtype=np.float32)
    for p, (i, j) in enumerate(pairs):
        c = confidence[p]
        conf[i, j] = conf[j, i] = c
        conf[i, i] = np.float32(conf[i, i] + np.float32(c / np.float32(2)))
        conf[j, j] = np.float32(conf[j, j] + np.float32(c / np.float32(2)))
    for j in range(v):
        # The float32 column sum in the order of torch's CPU kernel, which the reference's `conf.sum(dim=1)` runs and the records are
        # of: columns in groups of four are summed row by row; the columns left over (j >= 4 when v is 5, 6 or 7) and all eight
        # columns of v = 8 (the vectorised path) take four interleaved partial sums over the rows 4 m + k, the rows left over added
        # to the first, then ((p0 + p1) + p2) + p3.  Up to four views both are the sum in order.  One float32 ulp in a column sum
        # moves the result by about 1e-6: the records pin the order.
        part = np.zeros(4, dtype=np.float32)
        if v == 8 or j >= 4:
            for m in range(v // 4):
                for k in range(4):
                    part[k] = np.float32(part[k] + conf[4 * m + k, j])
            for i in range(4 * (v // 4), v):
                part[0] = np.float32(part[0] + conf[i, j])
        else:
            for i in range(v):
                part[0] = np.float32(part[0] + conf[i, j])
        total = np.float32(np.float32(np.float32(part[0] + part[1]) + part[2]) + part[3])
        conf[:, j] = conf[:, j] / np.maximum(total, np.float32(1e-9))
    L = np.zeros((4 * v, 4 * v), dtype=np.float32)
    for i in range(v):
        L[4 * i:4 * i + 4, 4 * i:4 * i + 4] = conf[i, i] * np.eye(4, dtype=np.float32)
    for p, (i, j) in enumerate(pairs):
        L[4 * i:4 * i + 4, 4 * j:4 * j + 4] = conf[i, j] * _se3_inverse_f32(Ps[p])
        L[4 * j:4 * j + 4, 4 * i:4 * i + 4] = conf[j, i] * Ps[p]
    L = L.astype(np.float64)
    for _ in range(squares):
        L = L @ L
    col = L.reshape(v, 4, v, 4)[:, :, 0, :]
    mass = col[:, 3, 3]
    if mass.min() == 0:
        return camera_chaining(Ps, v).astype(np.float64)
    col = col / np.maximum(mass, 1e-9)[:, None, None]
    out = col.copy()
    for i in range(v):
        U, _, Vt = np.linalg.svd(col[i, :3, :3])
        out[i, :3, :3] = (U * np.array([1.0, 1.0, np.linalg.det(U @ Vt)])) @ Vt
    return out
