"""The coarse camera poses (pf3plat_amd.pose; gsr_pnp_ransac / gsr_camera_sync; definition: include/gsr.h).

Yardsticks: for the PnP part the definition and tests/pnp_ref.py's float64 restatement on planted scenes (OpenCV is not available:
docs/PARITY.md section 16) - the consensus set must EQUAL the planted one and the pose lie within ROT_BOUND / TRANS_BOUND of the
float64 optimum over it; for the synchronisation the reference's own `camera_synchronization`, recorded in
tests/golden/pose_sync_fixtures.npz (make_pose_sync_fixtures.py).

ROT_BOUND, TRANS_BOUND: 4 x the largest rotation error (radians) and translation error (relative to the list's mean depth) measured
on the MI355X over the planted lists below (docs/PARITY.md section 16 records the measurements); results are bit-stable from run to
run, the margin is for other compiler and driver versions.  Both are far below the 3e-3 at which an unrefined hypothesis would pass."""
import ctypes
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

from pf3plat_amd import _lib, pose
from pf3plat_amd.losses import PackedCorrespondences
from tests import pnp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "pose_sync_fixtures.npz")
SOLVER = os.path.join(os.path.dirname(_lib.SRC), "gsr_pnp_solver.h")
M = pose.MIN_MATCHES
INVALID = -1  # GSR_ERR_INVALID_ARGUMENT of include/gsr.h
ROT_BOUND = 4 * 1.85e-9    # measured: 1.848e-9 rad (edges[2], n = 65)
TRANS_BOUND = 4 * 3.72e-9  # measured: 3.714e-9 of the mean depth (edges[1], n = 63)
# name: (seed, b, v, specs per list (n, inlier share, noisy), lists behind the camera, lists of one repeated id)
SCENES = {
    "mixed": (5, 2, 3, ((0, 1.0, False), (M - 1, 1.0, False), (M + 1, 1.0, False), (64, 0.5, True), (257, 0.4, True), (1500, 0.4, True)), (), ()),
    "edges": (9, 2, 3, ((M, 1.0, False), (63, 0.5, True), (65, 0.5, True), (0, 1.0, False), (30, 1.0, False), (0, 1.0, False)), (), (4,)),
    "behind": (3, 1, 2, ((M, 1.0, False),), (0,), ()),
}
# The list behind the camera is as short as a list may be.  Its matches are exact, and the pose they came from - a solution of the P3P
# equations with negative depths - is what every hypothesis of four distinct matches finds; the depth test then scores it 0.  A
# hypothesis whose fourth match repeats one of the first three cannot choose, and may keep a solution IN FRONT of the camera, which
# explains three matches exactly and misses the fourth: in this list by 10.6 px or more (enumerated in float64 over all 4^4 draws).
# In a longer list, at 5 px in a 64 x 48 image, some such pose explains a fourth match by chance - a consensus that any RANSAC,
# OpenCV's included, would return, and no failure case of the definition.
FAILING = {"mixed": {0: pose.STATUS_TOO_FEW_MATCHES, 1: pose.STATUS_TOO_FEW_MATCHES},
           "edges": {3: pose.STATUS_TOO_FEW_MATCHES, 4: pose.STATUS_NO_CONSENSUS, 5: pose.STATUS_TOO_FEW_MATCHES},
           "behind": {0: pose.STATUS_NO_CONSENSUS}}


@functools.lru_cache(maxsize=None)
def scene(name):
    seed, b, v, specs, behind, repeated = SCENES[name]
    sc = ref.build_scene(seed, b, v, specs, behind=behind)
    for l in repeated:
        ref.repeated_id_list(sc, l, specs[l][0], 777)
    return sc


@functools.lru_cache(maxsize=None)
def optimum(name, l):
    sc = scene(name)
    return sc.optimum(sc.lists[l])


def offsets_of(sc, only=None):
    lengths = [ls.ids_i.size if only is None or l == only else 0 for l, ls in enumerate(sc.lists)]
    return tuple(int(x) for x in np.cumsum([0] + lengths))


def pack(sc, dev, only=None):
    """The scene's lists as a PackedCorrespondences on `dev`; `only`: every other list emptied (a single-list call that keeps the
    list's index, which the draws depend on)."""
    keep = [ls for l, ls in enumerate(sc.lists) if only is None or l == only]
    cat = lambda k, dt: torch.from_numpy(np.concatenate([getattr(ls, k) for ls in keep]).astype(dt)).to(dev)
    offsets = offsets_of(sc, only)
    packed = PackedCorrespondences(cat("ids_i", np.int64), cat("ids_j", np.int64), cat("scores", np.float32),
                                   torch.zeros(len(sc.lists), dtype=torch.float32, device=dev), offsets,
                                   torch.tensor(offsets, dtype=torch.int32).to(dev), sc.b, len(sc.lists) // sc.b)
    return packed, cat("points_2d", np.float32)


def run(sc, dev, only=None, points=True, **kw):
    packed, pts = pack(sc, dev, only)
    out = pose.coarse_poses(torch.from_numpy(sc.xyz).to(dev), torch.from_numpy(sc.intrinsics).to(dev), packed,
                            points_2d=pts if points else None, return_mask=True, **kw)
    return {k: getattr(out, k).cpu().numpy() for k in ("pairwise", "absolute", "confidence", "inliers", "status", "mask")}


_RESULTS = {}


def result(name):
    if name not in _RESULTS:
        _RESULTS[name] = run(scene(name), torch.device("cuda"))
    return _RESULTS[name]


def pose_errors(sc, ls, pairwise, Ro, to):
    """Rotation error (radians) and translation error relative to the list's mean depth of the pose whose inverse `pairwise` is."""
    R = pairwise[:3, :3].astype(np.float64).T
    t = -R @ pairwise[:3, 3].astype(np.float64)
    D = R @ Ro.T
    sin = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    rot = np.arctan2(sin, (np.trace(D) - 1) / 2)
    depth = ref.project(Ro, to, sc.cam(ls), sc.points(ls)[ls.inlier])[1].mean()
    return rot, np.linalg.norm(t - to) / depth, depth


def planted_lists(name):
    return [l for l, ls in enumerate(scene(name).lists) if l not in FAILING[name]]


PLANTED = [(name, l) for name in SCENES for l in planted_lists(name)]


# ---- without a GPU ------------------------------------------------------------------------------------------------------------
def test_sync_restatement_reproduces_every_reference_record():
    with np.load(FIXTURES) as fx:
        names = [str(n) for n in fx["names"]]
        assert names == ["v2_b1", "v2_b2", "v3_b1", "v3_b2", "v4_b1", "v4_b2", "far_low", "zero", "v5_b2", "v6_b1", "v8_b1", "v8_b2", "zero_v5"]
        for name in names:
            Ps, conf, want, v = fx[name + "/pairwise"], fx[name + "/confidence"], fx[name + "/absolute"], int(fx[name + "/views"])
            b, pairs = Ps.shape[0], Ps.shape[1]
            assert want.dtype == np.float32 and want.shape == (b, v, 4, 4) and pairs == v * (v - 1) // 2
            for s in range(b):
                got = ref.camera_synchronization(Ps[s], conf[np.arange(pairs) * b + s], v).astype(np.float32)
                err = np.abs(got.astype(np.float64) - want[s].astype(np.float64)).max()
                print(f"{name}[{s}]: restatement vs record {err:.2e}")
                assert err <= 1e-12, (name, s, err)
        assert fx["far_low/means"][1] < 0.5 and fx["far_low/confidence"][1] == 0 and (fx["far_low/confidence"][[0, 2]] > 0).all()
        assert (fx["zero/confidence"] == 0).all() and fx["zero/pairwise"].shape[0] == 1
        chained = ref.camera_chaining(fx["zero/pairwise"][0], 3)
        assert np.array_equal(chained, fx["zero/absolute"][0])  # the record is of the fallback


@pytest.mark.parametrize("name,l", PLANTED)
def test_cases_exercise_what_they_claim(name, l):
    """Conditions on the inputs, at the float64 optimum over the planted inliers: every planted inlier reprojects within 2.5 px,
    every outlier lies beyond 10 px, all depths are positive, and a mixed list has at least 8 x MIN_MATCHES inliers."""
    sc = scene(name)
    ls = sc.lists[l]
    Ro, to = optimum(name, l)
    uv, z = ref.project(Ro, to, sc.cam(ls), sc.points(ls))
    err = np.linalg.norm(uv - ls.points_2d.astype(np.float64), axis=1)
    worst_in, nearest_out = err[ls.inlier].max(), (err[~ls.inlier].min() if (~ls.inlier).any() else np.inf)
    print(f"{name}[{l}] n={err.size}: inliers within {worst_in:.3f} px, outliers beyond {nearest_out:.3f} px")
    assert worst_in <= 2.5 and nearest_out >= 10.0 and (z > 0).all()
    assert ls.ids_i.min() >= 0 and ls.ids_i.max() < ref.H * ref.W and ls.ids_j.min() >= 0 and ls.ids_j.max() < ref.H * ref.W
    if not ls.inlier.all():
        assert ls.inlier.sum() >= 8 * M
    else:
        assert worst_in <= 1e-4  # exact matches but for the float32 rounding of the inputs


def test_scenes_cover_the_sizes_and_the_corner_ids():
    lengths = sorted(ls.ids_i.size for name in SCENES for l, ls in enumerate(scene(name).lists) if l not in FAILING[name])
    assert lengths == sorted([M, M + 1, 63, 64, 65, 257, 1500])
    corner = [ls for name in SCENES for ls in scene(name).lists if (ls.ids_j == 0).any() and (ls.ids_j == ref.H * ref.W - 1).any()
              and (ls.ids_i == 0).any() and (ls.ids_i == ref.H * ref.W - 1).any()]
    assert len(corner) >= 2
    sc = scene("behind")
    behind = sc.lists[0]
    assert (ref.project(behind.R, behind.t, sc.cam(behind), sc.points(behind))[1] < 0).all()
    assert np.unique(scene("edges").lists[4].ids_j).size == 1


def test_symbols_are_declared_exported_and_listed():
    import pf3plat_amd

    for name in ("coarse_poses", "pnp_ransac", "synchronize_cameras", "pack_matches", "CoarsePoses"):
        assert getattr(pf3plat_amd, name) is getattr(pose, name)
    lib = _lib.load()
    assert lib.gsr_abi_version() == 5 == _lib.GSR_ABI_VERSION
    assert lib.gsr_pnp_min_matches() == pose.MIN_MATCHES
    exported = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    assert "#define GSR_ABI_VERSION 5" in header
    for name in ("gsr_pnp_ransac", "gsr_pnp_ransac_scratch_bytes", "gsr_pnp_min_matches", "gsr_camera_sync"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(exported, name) and f"{name}(" in header, name
    assert lib.gsr_pnp_ransac.restype is ctypes.c_int and len(lib.gsr_pnp_ransac.argtypes) == 24
    assert lib.gsr_camera_sync.restype is ctypes.c_int and len(lib.gsr_camera_sync.argtypes) == 6
    kernels = os.path.join(os.path.dirname(_lib.SRC), "gsr_coarse_pose.h")
    assert "k_pnp_hypotheses" in open(kernels).read() and kernels in _lib.hip_sources()  # the content stamp of the build covers the kernels
    for path in _lib.hip_sources():  # the solver's header serves host and device as it is: no macro cuts a host build out of the library's text
        assert "GSR_POSE_HOST_ONLY" not in open(path).read(), path


def test_entry_points_refuse_invalid_sizes():
    """Every call below returns before a launch: nothing is read through the dummy pointer."""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def pnp(b=1, v=3, h=48, w=64, pairs=None, offsets=(0, 4, 8, 12), hyp=1000, thr=5.0, cmin=0.5, ptrs=None):
        pairs = v * (v - 1) // 2 if pairs is None else pairs
        host = (ctypes.c_int32 * len(offsets))(*offsets)
        a = ptrs or [p] * 13
        return lib.gsr_pnp_ransac(b, v, h, w, pairs, a[0], a[1], a[2], a[3], a[4], a[5], host, a[6], hyp, thr, cmin, 0, a[7], a[8], a[9], a[10],
                                  a[11], a[12], None)

    assert pnp(v=1, pairs=0, offsets=(0,)) == INVALID
    assert pnp(v=9, offsets=tuple(range(37))) == INVALID
    assert pnp(hyp=0) == INVALID and pnp(hyp=-5) == INVALID and pnp(hyp=(1 << 24) + 1) == INVALID
    assert pnp(offsets=(0, 4, 3, 12)) == INVALID and pnp(offsets=(-1, 4, 8, 12)) == INVALID
    assert pnp(pairs=2) == INVALID and pnp(b=-1) == INVALID and pnp(h=0) == INVALID and pnp(w=0) == INVALID and pnp(h=1 << 16, w=1 << 16) == INVALID
    assert pnp(thr=0.0) == INVALID and pnp(thr=float("nan")) == INVALID and pnp(cmin=1.0) == INVALID
    for k in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11):  # all but points_2d (5) and mask (12)
        assert pnp(ptrs=[None if q == k else p for q in range(13)]) == INVALID, k
    assert pnp(b=0, offsets=(0,)) == 0  # no scene: nothing is launched
    assert lib.gsr_pnp_ransac_scratch_bytes(2, 3, 1000) == 6 * 4 * 8 and lib.gsr_pnp_ransac_scratch_bytes(1, 2, 256) == 8
    for bad in ((1, 1, 1000), (1, 9, 1000), (1, 3, 0), (-1, 3, 10)):
        assert lib.gsr_pnp_ransac_scratch_bytes(*bad) == 0, bad
    for bad in ((1, 1), (1, 9), (-1, 3)):
        assert lib.gsr_camera_sync(*bad, p, p, p, None) == INVALID, bad
    for k in range(3):
        assert lib.gsr_camera_sync(1, 3, *[None if q == k else p for q in range(3)], None) == INVALID, k
    assert lib.gsr_camera_sync(0, 3, p, p, p, None) == 0


def test_python_checks_fire_in_order_and_refuse_cpu_tensors(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the checks were through")

    monkeypatch.setattr(_lib, "load", no_load)
    sc = scene("edges")
    packed, pts = pack(sc, torch.device("cpu"))
    xyz, k = torch.from_numpy(sc.xyz), torch.from_numpy(sc.intrinsics)
    bad = [((xyz[0], k, packed), {}, "xyz"), ((xyz[:, :1], k[:, :1], packed), {}, "views"), ((xyz, k[:, :2], packed), {}, "intrinsics_px"),
           ((xyz[:1], k[:1], packed), {}, "packed for"), ((xyz, k, packed), {"points_2d": pts[:-1]}, "points_2d"),
           ((xyz, k, packed), {"hypotheses": 0}, "hypotheses"), ((xyz, k, packed), {"reprojection_error": 0.0}, "reprojection_error"),
           ((xyz, k, packed), {"confidence_min": 1.0}, "confidence_min")]
    for args, kw, word in bad:
        with pytest.raises(ValueError, match=word):
            pose.coarse_poses(*args, **kw)
    with pytest.raises(ValueError, match="views"):
        pose.coarse_poses(xyz.repeat(1, 3, 1, 1, 1), k.repeat(1, 3, 1, 1), packed)  # 9 views
    with pytest.raises(RuntimeError, match="ROCm device"):  # the shapes are right: the device check is next
        pose.coarse_poses(xyz, k, packed, points_2d=pts)
    with pytest.raises(RuntimeError, match="ROCm device"):
        pose.pnp_ransac(xyz, k, packed)
    pw, cf = torch.eye(4).repeat(2, 3, 1, 1), torch.ones(6)
    for args, word in (((pw, cf, 1), "views"), ((pw, cf, 9), "views"), ((pw, cf, 4), "pairwise"), ((pw[0], cf, 3), "pairwise"), ((pw, cf[:5], 3), "confidence")):
        with pytest.raises(ValueError, match=word):
            pose.synchronize_cameras(*args)
    with pytest.raises(RuntimeError, match="ROCm device"):
        pose.synchronize_cameras(pw, cf, 3)


def test_pack_matches_is_pack_correspondences_without_confidences():
    from pf3plat_amd.losses import pack_correspondences

    sc = scene("edges")
    pairs = ref.pairs_of(sc.v)
    corr = {p: [tuple(torch.from_numpy(getattr(sc.lists[k * sc.b + s], f)) for f in ("ids_i", "ids_j", "scores")) for s in range(sc.b)]
            for k, p in enumerate(pairs)}
    got = pose.pack_matches(corr)
    conf = {p: torch.full((sc.b,), 0.25) for p in pairs}
    want = pack_correspondences(corr, conf)
    for f in ("ids_i", "ids_j", "weights", "offsets_device"):
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    assert got.offsets == want.offsets == offsets_of(sc) and (got.num_scenes, got.num_pairs) == (sc.b, len(pairs))
    assert torch.equal(got.conf, torch.zeros(len(pairs) * sc.b))
    assert torch.equal(dataclasses.replace(got, conf=want.conf).conf, want.conf)


HOST_WRAPPER = """
#include "%s"
using namespace gsr::pnp;
extern "C" int host_quartic(const double* c, double* roots) { return quartic_real_roots(c, roots); }
extern "C" int host_hypothesis(const double* X, const double* u, const double* K, double* out) {
  double XX[4][3], uu[4][2];
  for (int i = 0; i < 4; ++i) { for (int c = 0; c < 3; ++c) XX[i][c] = X[3 * i + c]; uu[i][0] = u[2 * i]; uu[i][1] = u[2 * i + 1]; }
  Camera cam{K[0], K[1], K[2], K[3]};
  Pose P;
  const bool ok = hypothesis(XX, uu, cam, &P);
  for (int i = 0; i < 9; ++i) out[i] = P.R[i];
  for (int i = 0; i < 3; ++i) out[9 + i] = P.t[i];
  return ok;
}
extern "C" void host_gauss_newton(int n, const double* X, const double* u, const double* K, double* pose, int steps) {
  Camera cam{K[0], K[1], K[2], K[3]};
  Pose P;
  for (int i = 0; i < 9; ++i) P.R[i] = pose[i];
  for (int i = 0; i < 3; ++i) P.t[i] = pose[9 + i];
  for (int s = 0; s < steps; ++s) {
    double acc[27] = {0};
    for (int k = 0; k < n; ++k) gn_accumulate(P, cam, X + 3 * k, u + 2 * k, acc);
    gn_step(&P, acc);
  }
  for (int i = 0; i < 9; ++i) pose[i] = P.R[i];
  for (int i = 0; i < 3; ++i) pose[9 + i] = P.t[i];
}
"""


def test_host_build_of_the_solver_in_float64(tmp_path):
    """The minimal solver and the Gauss-Newton step are host + device code: the same text, built for the host, finds the roots of a
    quartic, the planted pose of exact matches, and the float64 optimum of a noisy list."""
    import shutil
    import subprocess

    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler (the build needs one as well)"
    src, lib_path = tmp_path / "host_pnp.cpp", tmp_path / "host_pnp.so"
    src.write_text(HOST_WRAPPER % SOLVER)  # (the header is the host + device arithmetic alone and needs nothing else)
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(lib_path)], check=True)
    host = ctypes.CDLL(str(lib_path))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    roots = np.zeros(4)
    coeffs = np.poly([1.0, 2.0, -3.0, 0.5])[::-1].copy() * -1.7  # c[0] + c[1] y + ... + c[4] y^4
    assert host.host_quartic(ptr(coeffs), ptr(roots)) == 4 and np.allclose(np.sort(roots), [-3.0, 0.5, 1.0, 2.0], atol=1e-12)
    coeffs = np.poly([1.0, 2.0, 0.3 + 0.4j, 0.3 - 0.4j]).real[::-1].copy()
    assert host.host_quartic(ptr(coeffs), ptr(roots)) == 2 and np.allclose(np.sort(roots[:2]), [1.0, 2.0], atol=1e-12)
    sc = scene("edges")
    ls = sc.lists[0]  # four exact matches
    X, u, cam = np.ascontiguousarray(sc.points(ls)), np.ascontiguousarray(ls.points_2d.astype(np.float64)), np.array(sc.cam(ls))
    found = np.zeros(12)
    assert host.host_hypothesis(ptr(X), ptr(u), ptr(cam), ptr(found)) == 1
    Ro, to = optimum("edges", 0)
    assert np.abs(found[:9].reshape(3, 3) - Ro).max() <= 1e-6 and np.abs(found[9:] - to).max() <= 1e-5
    ls = sc.lists[2]  # 65 matches, 33 noisy inliers: thirty steps from the planted pose reach the optimum
    m = ls.inlier
    X, u = np.ascontiguousarray(sc.points(ls)[m]), np.ascontiguousarray(ls.points_2d[m].astype(np.float64))
    state = np.concatenate([ls.R.reshape(-1), ls.t])
    host.host_gauss_newton(int(m.sum()), ptr(X), ptr(u), ptr(np.array(sc.cam(ls))), ptr(state), 30)
    Ro, to = optimum("edges", 2)
    assert np.abs(state[:9].reshape(3, 3) - Ro).max() <= 1e-12 and np.abs(state[9:] - to).max() <= 1e-12


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,l", PLANTED)
def test_consensus_set_equals_the_planted_one_and_the_pose_the_optimum(name, l):
    sc, out = scene(name), result(name)
    ls = sc.lists[l]
    lo, hi = offsets_of(sc)[l], offsets_of(sc)[l + 1]
    assert out["status"][l] == pose.STATUS_OK
    assert np.array_equal(out["mask"][lo:hi].astype(bool), ls.inlier), (name, l)  # EQUAL: no exception is allowed
    assert out["inliers"][l] == ls.inlier.sum()
    pw = out["pairwise"][ls.scene, l // sc.b]
    assert np.array_equal(pw[3], np.array([0, 0, 0, 1], dtype=np.float32))
    Ro, to = optimum(name, l)
    rot, trans, depth = pose_errors(sc, ls, pw, Ro, to)
    print(f"MEASURED {name}[{l}] n={ls.ids_i.size}: rotation {rot:.3e} rad, translation {trans:.3e} of the mean depth {depth:.2f}")
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Ro, to
    assert np.abs(pw.astype(np.float64) @ T - np.eye(4)).max() <= 1e-6 + ROT_BOUND + TRANS_BOUND * depth
    assert rot <= ROT_BOUND and trans <= TRANS_BOUND, (rot, trans)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_failure_paths_give_identity_and_the_documented_status(name):
    sc, out = scene(name), result(name)
    off = offsets_of(sc)
    for l, status in FAILING[name].items():
        ls = sc.lists[l]
        assert out["status"][l] == status and out["inliers"][l] == 0, (l, out["status"][l], out["inliers"][l])
        assert np.array_equal(out["pairwise"][ls.scene, l // sc.b], np.eye(4, dtype=np.float32)), l
        assert not out["mask"][off[l]:off[l + 1]].any()
    want = ref.expected_confidence(sc)
    assert np.isfinite(out["confidence"]).all()
    assert np.abs(out["confidence"] - want).max() <= 4 * np.finfo(np.float32).eps, (out["confidence"], want)
    for l, ls in enumerate(sc.lists):
        if ls.ids_i.size == 0:
            assert out["confidence"][l] == 0  # where the reference has NaN


@pytest.mark.gpu
def test_one_call_with_mixed_lists_equals_single_list_calls():
    sc, out = scene("mixed"), result("mixed")
    off = offsets_of(sc)
    assert [off[l + 1] - off[l] for l in range(6)] == [0, M - 1, M + 1, 64, 257, 1500]
    dev = torch.device("cuda")
    for l, ls in enumerate(sc.lists):
        one = run(sc, dev, only=l)
        assert np.array_equal(one["pairwise"][ls.scene, l // sc.b], out["pairwise"][ls.scene, l // sc.b]), l
        assert one["inliers"][l] == out["inliers"][l] and one["status"][l] == out["status"][l] and one["confidence"][l] == out["confidence"][l]
        assert np.array_equal(one["mask"], out["mask"][off[l]:off[l + 1]]), l


@pytest.mark.gpu
def test_repeated_call_same_bits_other_seed_same_mask_points_as_pixels():
    sc, out = scene("mixed"), result("mixed")
    dev = torch.device("cuda")
    again = run(sc, dev)
    for k in out:
        assert np.array_equal(again[k], out[k], equal_nan=True), k
    other = run(sc, dev, seed=12345)
    assert np.array_equal(other["mask"], out["mask"]) and np.array_equal(other["status"], out["status"])
    for l in planted_lists("mixed"):
        ls = sc.lists[l]
        rot, trans, _ = pose_errors(sc, ls, other["pairwise"][ls.scene, l // sc.b], *optimum("mixed", l))
        print(f"MEASURED other seed mixed[{l}]: rotation {rot:.3e} rad, translation {trans:.3e}")
        assert rot <= ROT_BOUND and trans <= TRANS_BOUND, (l, rot, trans)
    # points_2d equal to the pixels of ids_i: the same bits as None
    packed, _ = pack(sc, dev)
    pix = torch.stack([packed.ids_i % ref.W, packed.ids_i // ref.W], 1).to(torch.float32)
    xyz, k = torch.from_numpy(sc.xyz).to(dev), torch.from_numpy(sc.intrinsics).to(dev)
    a = pose.pnp_ransac(xyz, k, packed, points_2d=pix, return_mask=True)
    b = pose.pnp_ransac(xyz, k, packed, return_mask=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not any(t.requires_grad for t in a)


@pytest.mark.gpu
def test_synchronisation_agrees_with_the_reference_records():
    dev = torch.device("cuda")
    with np.load(FIXTURES) as fx:
        rec = {k: fx[k] for k in fx.files}
    for name in [str(n) for n in rec["names"]]:
        v = int(rec[name + "/views"])
        got = pose.synchronize_cameras(torch.from_numpy(rec[name + "/pairwise"]).to(dev), torch.from_numpy(rec[name + "/confidence"]).to(dev), v)
        assert got.dtype == torch.float32 and not got.requires_grad
        u = ref.ulps(got.cpu().numpy(), rec[name + "/absolute"])
        print(f"MEASURED sync {name}: {u:.2f} ulps")
        assert u <= 4, (name, u)
    # the fallback scene batched with a normal one: each as its own b = 1 record (the decision is per scene)
    Ps = np.concatenate([rec["v3_b1/pairwise"], rec["zero/pairwise"]])
    conf = np.stack([rec["v3_b1/confidence"], rec["zero/confidence"]], 1).reshape(-1)  # list order: pair-major
    got = pose.synchronize_cameras(torch.from_numpy(Ps).to(dev), torch.from_numpy(conf).to(dev), 3).cpu().numpy()
    assert ref.ulps(got[:1], rec["v3_b1/absolute"]) <= 4 and ref.ulps(got[1:], rec["zero/absolute"]) <= 4
    assert np.array_equal(got[1, 0], np.eye(4, dtype=np.float32))


@pytest.mark.gpu
def test_coarse_poses_is_pnp_ransac_then_synchronize_cameras():
    sc, out = scene("mixed"), result("mixed")
    dev = torch.device("cuda")
    packed, pts = pack(sc, dev)
    xyz, k = torch.from_numpy(sc.xyz).to(dev), torch.from_numpy(sc.intrinsics).to(dev)
    pw, inl, st, mask = pose.pnp_ransac(xyz, k, packed, points_2d=pts, return_mask=True)
    assert np.array_equal(pw.cpu().numpy(), out["pairwise"]) and np.array_equal(inl.cpu().numpy(), out["inliers"])
    assert np.array_equal(st.cpu().numpy(), out["status"]) and np.array_equal(mask.cpu().numpy(), out["mask"])
    assert len(pose.pnp_ransac(xyz, k, packed, points_2d=pts)) == 3
    absolute = pose.synchronize_cameras(pw, torch.from_numpy(out["confidence"]).to(dev), sc.v)
    assert np.array_equal(absolute.cpu().numpy(), out["absolute"])
    assert np.isfinite(out["absolute"]).all() and np.array_equal(out["absolute"][:, 0, 3], np.tile(np.array([0, 0, 0, 1], dtype=np.float32), (sc.b, 1)))


@pytest.mark.gpu
def test_the_chain_runs_without_a_host_synchronisation():
    sc = scene("mixed")
    dev = torch.device("cuda")
    packed, pts = pack(sc, dev)
    xyz, k = torch.from_numpy(sc.xyz).to(dev), torch.from_numpy(sc.intrinsics).to(dev)
    pose.coarse_poses(xyz, k, packed, points_2d=pts)  # (the library is loaded, the allocator warm)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:  # noqa: BLE001
        pytest.skip(f"this torch build has no synchronisation debug mode on ROCm: {e}")
    try:
        try:
            xyz.sum().item()
            caught = False
        except RuntimeError:
            caught = True
        if not caught:
            torch.cuda.set_sync_debug_mode("default")
            pytest.skip("this torch build's synchronisation debug mode does not report a synchronising call on ROCm")
        out = pose.coarse_poses(xyz, k, packed, points_2d=pts, return_mask=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(out.pairwise.cpu().numpy(), result("mixed")["pairwise"])
