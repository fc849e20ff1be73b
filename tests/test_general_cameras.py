"""CPU guards of the cases tests/test_gpu_general_cameras.py renders (tests/camera_rig.py CASES): every one meets the seed guard - the fp32
oracle against the fp64 oracle through parity_checks with 0 outlier pixels, 0 flipped pixels and nothing set aside, so a strict failure
on the device is never the reference's own threshold flip - and the rig delivers what it is for: rolled, per-view, anisotropic cameras
with Gaussians behind them and beyond the frustum clamp."""
import functools

import numpy as np
import pytest

from pf3plat_amd import synthetic
from tests import camera_rig, gpu_util


@functools.lru_cache(maxsize=None)
def _oracle_radii(name):
    c = camera_rig.case(name)
    o = gpu_util.run_oracle(*c.args(), oracle_dtype=np.float32, frames=c.frames, sh_frame=c.sh_frame)
    return camera_rig.population(c, o["radii"])


def test_general_cameras_is_a_pure_function_of_the_seed_and_keeps_the_gaussians():
    sc = synthetic.make_scene(3, 50, (16, 16), num_views=3)
    a, b, other = camera_rig.general_cameras(sc, 9), camera_rig.general_cameras(sc, 9), camera_rig.general_cameras(sc, 10)
    for name in ("extrinsics", "intrinsics", "near", "far"):
        assert np.array_equal(getattr(a, name).numpy(), getattr(b, name).numpy()), name
    assert not np.array_equal(a.extrinsics.numpy(), other.extrinsics.numpy())
    assert a.gaussians is sc.gaussians and a.extrinsics.shape == (1, 3, 4, 4) and a.near.shape == (1, 3)
    assert float(a.far.min()) == 100.0 and set(a.near.reshape(-1).tolist()) <= set(camera_rig.NEARS)
    ext = a.extrinsics[0].double().numpy()
    for v in range(3):  # proper rigid poses
        r = ext[v, :3, :3]
        assert np.abs(r @ r.T - np.eye(3)).max() < 1e-6 and np.linalg.det(r) > 0.999 and np.array_equal(ext[v, 3], [0, 0, 0, 1])
    # what the rig replaces: make_scene's own rotations are exactly I
    assert np.array_equal(sc.extrinsics[0, :, :3, :3].numpy(), np.broadcast_to(np.eye(3, dtype=np.float32), (3, 3, 3)))


@pytest.mark.parametrize("name", list(camera_rig.CASES))
def test_case_meets_the_seed_guard(name):
    """fp32 oracle vs fp64 oracle: check_image, check_grads and check_camera_grads with no outlier, no flip, nothing set aside."""
    c = camera_rig.case(name)
    m = (camera_rig.alpha_guard if c.cfg.alpha else camera_rig.seed_guard)(c)
    assert m["means_norm"] > 0 and m["colors_norm"] > 0
    if c.want_views:
        assert 0.0 < m["camera_worst"] < 1e-5


@pytest.mark.parametrize("name", list(camera_rig.CASES))
def test_case_has_the_rig_properties(name):
    """Every view: six non-zero off-diagonal rotation entries (>= 0.01), fx and fy at least 5 % apart; no two views of the call share a
    rotation or a tangent pair, no two views of a set a near plane or - under the scale-invariant rescale - a scale."""
    c = camera_rig.case(name)
    camera_rig.rig_properties(c)
    assert c.cfg.num_gaussians <= 6000 and max(c.cfg.height, c.cfg.width) <= 96


def test_seeds_are_distinct():
    seeds = [kw["seed"] for kw in camera_rig.CASES.values()]
    assert len(set(seeds)) == len(seeds)


def test_the_cases_have_culled_gaussians_and_gaussians_beyond_the_frustum_clamp():
    """Across the module's cases: views with Gaussians that the z <= 0.2 test culls (behind the camera or inside the near cull: one test
    in the kernels), and views with visible Gaussians beyond the 1.3 tan-fov clamp (the population table of docs/PARITY.md section 9 is
    this, per case)."""
    culled = clamped = 0
    for name in camera_rig.CASES:
        rows = _oracle_radii(name)
        n = camera_rig.CASES[name].get("n", 3000)
        print(name, " | ".join(f"visible {r['visible']} behind {r['behind']} near {r['near_culled']} clamped {r['clamped']}" for r in rows))
        for r in rows:
            assert 0 < r["visible"] <= n - r["behind"] - r["near_culled"], (name, r)
        culled += sum(r["behind"] + r["near_culled"] > 0 for r in rows)
        clamped += sum(r["clamped"] > 0 for r in rows)
    assert culled >= 1 and clamped >= 1, (culled, clamped)
    assert max(r["near_culled"] + r["behind"] for r in _oracle_radii("a_culled")) >= 5


def test_the_fp64_floor_is_the_oracles_own_figure():
    """camera_rig.FP64_FLOOR is measured on the reference, never on the kernels: the largest distance of the fp32 oracle's dL/dviewmatrix
    from the fp64 oracle's over the committed cases with camera gradients, the oracle on one thread (one fixed order of its sums)."""
    from tests.util import rel_l2

    worst = 0.0
    for name, kw in camera_rig.CASES.items():
        if not kw.get("want_views") or kw.get("alpha"):
            continue
        c = camera_rig.case(name)
        run = lambda dt: gpu_util.run_oracle(*c.args(), c.gc, c.ge, dt, True, c.want_views, c.frames, c.sh_frame, threads=1)["grads"]["views"]
        worst = max(worst, rel_l2(run(np.float32)[:, :16], run(np.float64)[:, :16]))
    # (the floor may not exceed what the reference measures, nor be a stale leftover of other cases)
    assert 0.5 * worst <= camera_rig.FP64_FLOOR["dL/dviewmatrix"] <= 1.02 * worst, worst
