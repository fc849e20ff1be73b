"""Parity on the MI355X under general cameras (tests/camera_rig.py): every view a rigid pose of its own with roll, its own anisotropic field
of view and its own near plane, Gaussians inside the z <= 0.2 cull and beyond the frustum clamp.  The rest of the GPU suite renders through
`synthetic.make_scene`'s cameras - rotation exactly I in every view, fx = fy, one near per scene - where a transposed view matrix, view
0's rotation read for every view of a set or tan-fov x for y return the same bits.

Every case is named in camera_rig.CASES and held, on the CPU (tests/test_general_cameras.py), to the seed guard: the fp32 oracle against
the fp64 oracle passes the same checks with no outlier pixel, no flipped pixel and nothing set aside.  Here: HIP against the fp32 oracle
on the same record bits, strict (rel-L2 < 1e-4 over ALL pixels and ALL gradient rows), per-view stage checks, camera gradients per view
and block; HIP against the fp64 oracle within twice the fp32 oracle's own distance (docs/PARITY.md section 9 has the table and the
mutations these tests were measured against); and the torch-facing wrappers over HipBackend against the same wrappers over the oracle,
with the whole of `extrinsics.grad` compared."""
import numpy as np
import pytest
import torch

import pf3plat_amd
from pf3plat_amd import _lib, rasterizer
from pf3plat_amd.types import Gaussians
from tests import camera_rig, gpu_util, parity_checks
from tests.camera_rig import MODES, case
from tests.oracle_backend import OracleBackend
from tests.util import install_backend, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FOLLOWS, DET, WINDOWED = _lib.FLAG_BACKWARD_FOLLOWS, _lib.FLAG_DETERMINISTIC, _lib.FLAG_WINDOWED_BINNING


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(c, flags=0):
    """HIP and the fp32 oracle on case `c` (+ HIP-side flags that do not change what is computed)."""
    ch = c.with_flags(flags)
    return ch.cfg, gpu_util.run_both(ch.cfg, c.vb, c.means, c.cov, c.opac, c.colors, c.extra, c.gc, c.ge, want_views=c.want_views,
                                     frames=c.frames, sh_frame=c.sh_frame, rows_in_workspace=bool(flags & FOLLOWS))


def _hip(c, flags=0):
    ch = c.with_flags(flags)
    return gpu_util.run_hip(ch.cfg, c.vb, c.means, c.cov, c.opac, c.colors, c.extra, c.gc, c.ge, frames=c.frames, sh_frame=c.sh_frame,
                            want_views=c.want_views)


def _strict(c, cfg, res):
    """Every stage check per view (all tiles), the image and the gradients over ALL pixels and rows, the camera gradients."""
    assert not res["hip"]["status"]["overflow"]
    parity_checks.all_checks(cfg, res, lists=True, max_tiles=None, strict=True)
    if cfg.has_extra:
        assert rel_l2(res["hip"]["extra"], res["oracle"]["extra"]) < parity_checks.TOL
    if c.want_views:
        worst = parity_checks.check_camera_grads(res)
        assert worst < parity_checks.TOL
        assert all(np.abs(res["hip"]["grads"]["views"][v]).max() > 0 for v in range(cfg.num_views))
    return res


# ---- a: three views of one set ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a_sh4_extra", "a_sh0", "a_sh1", "a_sh2", "a_sh3", "a_rgb"])
def test_three_views_of_one_set(name):
    c = case(name)
    cfg, res = _run(c)
    _strict(c, cfg, res)
    assert all(st.n_visible > 1500 for st in res["oracle"]["stats"])


def test_gaussians_inside_the_cull_get_no_gradient_from_that_view():
    """`a_culled`: 20 Gaussians fail the z <= 0.2 test in the second of two views and pass it in the first; degree-4 harmonics, built-in
    depth, camera gradients.  Their radius in that view is 0 on both sides and their screen-space gradient row exactly 0."""
    c = case("a_culled")
    cfg, res = _run(c)
    _strict(c, cfg, res)
    pop = camera_rig.population(c, res["oracle"]["radii"])
    assert pop[1]["near_culled"] + pop[1]["behind"] >= 5
    f = c.vb[1].numpy()
    m = c.means[0].numpy() * f[40]
    culled = (f[2] * m[:, 0] + f[6] * m[:, 1] + f[10] * m[:, 2] + f[14]) <= np.float32(0.2)
    assert culled.sum() == pop[1]["near_culled"] + pop[1]["behind"]
    assert not res["hip"]["radii"][1][culled].any() and not res["hip"]["grads"]["means2d"][1][culled].any()
    assert res["hip"]["radii"][0][culled].any()


# ---- b: several sets, every view its own camera -----------------------------------------------------------------------------------------
def test_two_sets_of_two_views_every_view_its_own_camera():
    c = case("b_two_sets")
    cfg, res = _run(c)
    _strict(c, cfg, res)


@pytest.mark.parametrize("det", [False, True])
def test_three_sets_in_one_call_equal_their_three_single_set_calls(det):
    """Three sets x two views, degree-4 harmonics, built-in depth, gradients including `views`: image, depth and radii bit for bit; the
    gradients bit for bit in deterministic mode (integer sums) and to the rounding of fp32 atomics in another order otherwise (max-abs
    within 1e-5 of the tensor's largest entry, as test_forward_is_deterministic_and_backward_nearly has it).  A kernel that read set
    0's cameras, or a set's first view, for the others would differ in the image already."""
    c = case("b_three_sets")
    flags = DET if det else 0
    whole = _hip(c, flags)
    assert not whole["status"]["overflow"] and np.abs(whole["grads"]["views"]).min(axis=0).max() > 0
    vps = c.cfg.views_per_set

    def same(a, b, what):
        if det:
            assert np.array_equal(_bits(a), _bits(b)), what
        else:
            assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max(), what

    for s in range(c.cfg.num_sets):
        one = _hip(c.set_slice(s), flags)
        v = slice(s * vps, (s + 1) * vps)
        for name in ("color", "extra"):
            assert np.array_equal(_bits(whole[name][v]), _bits(one[name])), (s, name)
        assert np.array_equal(whole["radii"][v], one["radii"]), s
        for name in ("means", "cov6", "opac", "colors"):
            same(whole["grads"][name][s:s + 1], one["grads"][name], (s, name))
        for name in ("means2d", "views"):
            same(whole["grads"][name][v], one["grads"][name], (s, name))
    for a in range(c.cfg.num_views):  # no two views of the call render the same image
        for b in range(a + 1, c.cfg.num_views):
            assert rel_l2(whole["color"][a], whole["color"][b]) > 1e-2, (a, b)


# ---- c: the built-in extra modes read the z row of a rotated view matrix and the per-view scale ---------------------------------------
@pytest.mark.parametrize("rescale", ["invariant", "plain"])
@pytest.mark.parametrize("mode", list(MODES))
def test_built_in_extra_modes(mode, rescale):
    c = case(f"c_{mode}_{rescale}")
    cfg, res = _run(c)
    _strict(c, cfg, res)
    assert np.abs(res["hip"]["extra"]).max() > 0
    scales = c.vb[:, 40].numpy()
    assert (scales[0] != scales[1]) if rescale == "invariant" else (scales == 1.0).all()


# ---- d: camera gradients, both accumulation modes, saved direction Jacobian or re-read harmonics ---------------------------------------
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("follows", [False, True])
@pytest.mark.parametrize("name", ["d_full", "d_depth"])
def test_camera_gradients(name, follows, det):
    """k_preprocess_bwd / k_preprocess_bwd_det at pose 1 (every term) and pose 2 (the depth channel's term alone)."""
    c = case(name)
    cfg, res = _run(c, (FOLLOWS if follows else 0) | (DET if det else 0))
    _strict(c, cfg, res)
    h = res["hip"]["grads"]["views"]
    if name == "d_depth":  # only the z row of the view matrix gets a gradient
        assert not h[:, [0, 1, 4, 5, 8, 9, 12, 13]].any() and not h[:, 16:35].any() and np.abs(h[:, [2, 6, 10, 14]]).min() > 0
    else:
        assert np.abs(h[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]]).min() > 0 and np.abs(h[:, 32:35]).min() > 0


# ---- e: scale / rotation records in frames; the view direction carried into a frame and its gradient back -------------------------------
@pytest.mark.parametrize("follows", [False, True])
@pytest.mark.parametrize("sh_frame", [None, "rasterizer", "e3nn"])
def test_scale_rotation_records_with_frames(sh_frame, follows):
    c = case(f"e_{sh_frame}")
    cfg, res = _run(c, FOLLOWS if follows else 0)
    _strict(c, cfg, res)
    assert np.abs(res["hip"]["grads"]["colors"][..., 1:]).max() > 0 and np.abs(res["hip"]["grads"]["views"][:, 32:35]).min() > 0


# ---- f: windowed binning (the stand-alone k_preprocess) against the fused one -----------------------------------------------------------
def test_windowed_binning_same_lists_identical_image_bits():
    c = case("f_windowed")
    out = {}
    for name, fl in (("fused", 0), ("windowed", WINDOWED)):
        cfg, res = _run(c, fl)
        out[name] = _strict(c, cfg, res)["hip"]
    assert np.array_equal(_bits(out["fused"]["color"]), _bits(out["windowed"]["color"]))
    assert np.array_equal(out["fused"]["radii"], out["windowed"]["radii"])
    wa, wb = out["fused"]["ws"], out["windowed"]["ws"]
    assert wa["num_pairs"] == wb["num_pairs"] and wa["max_list"] == wb["max_list"]
    for v in range(c.cfg.num_views):
        for t in range(wa["T"]):
            (a0, a1), (b0, b1) = wa["ranges"][v, t], wb["ranges"][v, t]
            np.testing.assert_array_equal(wa["point_list"][a0:a1], wb["point_list"][b0:b1])


# ---- g: the forward instances ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,flags,in_binning", [("g_colour_in_binning", 0, 1), ("g_plain", 0, 0), ("g_k_color", WINDOWED, 0)])
def test_forward_instances(name, flags, in_binning):
    """Colour inside the binning launch (k_preprocess_bin<colour>), the plain binning launch followed by k_color (five views per set: more
    than the binning launch's colour waves take), and k_color after the stand-alone k_preprocess of the windowed chain."""
    c = case(name)
    hip = rasterizer.HipBackend()
    assert hip.lib.gsr_colour_in_binning(hip._dims(c.with_flags(flags).cfg, 1 << 16)) == in_binning
    cfg, res = _run(c, flags)
    _strict(c, cfg, res)


# ---- h: accumulated alpha ---------------------------------------------------------------------------------------------------------------------
def test_accumulated_alpha_image_gradients_and_camera_gradients():
    from tests.test_alpha_gpu import check_all, hip_alpha

    c = case("h_alpha")
    ga, (o32, o64) = camera_rig.alpha_pair(c)
    tup = (c.cfg, c.vb, c.means, c.cov, c.opac, c.colors, c.extra, c.frames)
    h = hip_alpha(tup, c.gc, c.ge, ga, want_views=True)
    m = check_all(tup, h, o32, o64)
    assert m["outlier_pixels_1e-4"] == 0 and m["color_rel_l2_all"] < parity_checks.TOL
    parity_checks.assert_nothing_set_aside(m)
    assert parity_checks.check_camera_grads(dict(hip=h, oracle=o32)) < parity_checks.TOL
    h0 = hip_alpha(tup, c.gc, c.ge, torch.zeros_like(ga), want_views=True)
    assert not np.array_equal(h0["grads"]["views"], h["grads"]["views"])  # (the alpha term is in the camera gradients)


# ---- i: fp64 arbitration ------------------------------------------------------------------------------------------------------------------
ARBITRATED = ["a_sh4_extra", "a_sh0", "a_sh1", "a_sh2", "a_sh3", "a_rgb", "a_culled"] + [f"c_{m}_{r}" for m in MODES for r in ("invariant", "plain")] + \
    ["d_full", "d_depth"]


# dL/dviewmatrix: a view's sum over all its Gaussians, 16 numbers.  As the tests run it the fp32 oracle adds them up in eight threads
# and lands 3e-8 .. 8e-8 from fp64 on the arbitrated cases - at or below half an ulp (6e-8) rms, i.e. where the correctly rounded result
# is, and by the luck of which thread finishes first (the figure moves by a factor of two from run to run); on one thread, one sum after
# the other, it is 8e-8 .. 1.0e-6 away.  The kernels add per lane, across 16 lanes, then across workgroups (k_pose_reduce), a tree of
# fp32 sums that ends 1e-7 .. 1.7e-7 away, two or three ulp.  No fp32 sum in another order can be held to twice a figure that is the
# rounding of the result alone, so this tensor's bar is the larger of 2 x and the largest distance the fp32 oracle itself has from fp64
# for it over all the committed cases with camera gradients (camera_rig.FP64_FLOOR: measured on the reference, on one thread;
# tests/test_general_cameras.py re-measures it).
FP64_FLOOR = camera_rig.FP64_FLOOR


def three_columns(c, res, o64):
    """-> rows (tensor, HIP vs fp64, fp32 oracle vs fp64, HIP vs fp32 oracle), rel-L2 over all elements, as tools/parity_vs_fp64.py."""
    rows = []

    def add(name, hip, o32, ref):
        if hip is not None and ref is not None and np.linalg.norm(ref) > 0:
            rows.append((name, rel_l2(hip, ref), rel_l2(o32, ref), rel_l2(hip, o32)))

    add("image", res["hip"]["color"], res["oracle"]["color"], o64["color"])
    add("extra image", res["hip"]["extra"], res["oracle"]["extra"], o64["extra"])
    for k in ("means", "cov6", "opac", "colors", "extra", "means2d"):
        add("dL/d" + k, res["hip"]["grads"].get(k), res["oracle"]["grads"].get(k), o64["grads"].get(k))
    if c.want_views:
        hv, ov, rv = (r["grads"]["views"] for r in (res["hip"], res["oracle"], o64))
        for blk, lo, hi in (("viewmatrix", 0, 16), ("projmatrix", 16, 32), ("campos", 32, 35)):
            add("dL/d" + blk, hv[:, lo:hi], ov[:, lo:hi], rv[:, lo:hi])
    return rows


@pytest.mark.parametrize("name", ARBITRATED)
def test_hip_is_within_twice_the_fp32_oracles_distance_to_fp64(name):
    """Per tensor: rel-L2(HIP, fp64 oracle) <= 2 x rel-L2(fp32 oracle, fp64 oracle) on the same case - the factor of docs/PARITY.md
    section 7 (two correct fp32 evaluations in different association orders).  The three columns are printed; section 9 has them."""
    c = case(name)
    cfg, res = _run(c)
    o64 = gpu_util.run_oracle(*c.args(), c.gc, c.ge, np.float64, True, c.want_views, c.frames, c.sh_frame)
    rows = three_columns(c, res, o64)
    for tensor, a, b, ab in rows:
        print(f"| {name} | {tensor} | {a:.3e} | {b:.3e} | {ab:.3e} | {a / max(b, 1e-30):.2f} |")
    assert len(rows) >= 6
    over = [(t, a, b) for t, a, b, _ in rows if a > max(2.0 * b, FP64_FLOOR.get(t, 0.0))]
    assert not over, over


# ---- the torch-facing path: the wrappers over HipBackend against the same wrappers over the oracle ------------------------------------
def _with_oracle(fn):
    old = install_backend(OracleBackend(threads=8))
    try:
        return fn()
    finally:
        install_backend(old)


def _leafs(sc, device):
    g = sc.gaussians
    return [t.detach().clone().to(device).requires_grad_(True) for t in (g.means, g.covariances, g.harmonics, g.opacities)]


def _same_grads(a, b):
    for x, y in zip(a, b):
        assert float(y.grad.abs().max()) > 0 and rel_l2(x.grad.cpu().numpy(), y.grad.cpu().numpy()) < parity_checks.TOL


def test_render_cuda_under_the_rig():
    sc = case("b_two_sets").scenes[0]  # 2 cameras, 2000 Gaussians, 48 x 56
    hw, b = sc.image_shape, 2
    w = torch.rand((b, 3, *hw), generator=torch.Generator().manual_seed(1))

    def run(device):
        m, c, h, o = _leafs(sc, device)
        rep = lambda t: t.expand(b, *t.shape[1:])
        img = pf3plat_amd.render_cuda(sc.extrinsics[0].to(device), sc.intrinsics[0].to(device), sc.near[0].to(device), sc.far[0].to(device),
                                      hw, torch.tensor([[0.1, 0.2, 0.3]] * b, device=device), rep(m), rep(c), rep(h), rep(o))
        (img * w.to(device)).sum().backward()
        return img.detach().cpu().numpy(), (m, c, h, o)

    gi, gl = run(DEV)
    oi, ol = _with_oracle(lambda: run("cpu"))
    assert rel_l2(gi, oi) < parity_checks.TOL and rel_l2(gi[0], gi[1]) > 1e-2
    _same_grads(gl, ol)


@pytest.mark.parametrize("mode", list(MODES))
def test_render_depth_cuda_under_the_rig(mode):
    """Two rolled cameras over one copy of the Gaussians, `extrinsics` requiring grad: the depth render's own camera gradient, whole."""
    sc = case(f"c_{mode}_invariant").scenes[0]
    hw = sc.image_shape
    w = torch.rand((2, *hw), generator=torch.Generator().manual_seed(2))

    def run(device):
        m, c, h, o = _leafs(sc, device)
        ext = sc.extrinsics[0].clone().to(device).requires_grad_(True)
        d = pf3plat_amd.render_depth_cuda(ext, sc.intrinsics[0].to(device), sc.near[0].to(device), sc.far[0].to(device), hw, m, c, o, mode=mode)
        (d * w.to(device)).sum().backward()
        return d.detach().cpu().numpy(), (m, c, o), ext.grad.cpu().numpy()

    gd, gl, ge = run(DEV)
    od, ol, oe = _with_oracle(lambda: run("cpu"))
    assert gd.shape == (2, *hw) and rel_l2(gd, od) < parity_checks.TOL
    _same_grads(gl, ol)  # means, covariances, opacities (the means move the footprint in every mode)
    if mode == "log":  # (the reference's min(near).max(far).log() is a constant: no gradient through z, none for the camera)
        assert not ge.any() and not oe.any()
    else:
        _compare_extrinsics_grad(ge, oe)


def test_render_cuda_orthographic_under_the_rig():
    sc = case("a_rgb").scenes[0]
    g = sc.gaussians
    hw = (48, 64)

    def run(device):
        t = lambda x: x.to(device)
        return pf3plat_amd.render_cuda_orthographic(
            t(sc.extrinsics[0]), torch.tensor([6.0, 5.0, 7.0], device=device), torch.tensor([4.5, 6.0, 5.0], device=device),
            torch.zeros(3, device=device), torch.full((3,), 40.0, device=device), hw, torch.zeros((3, 3), device=device),
            *(t(x.expand(3, *x.shape[1:])) for x in (g.means, g.covariances, g.harmonics, g.opacities)), fov_degrees=10.0).cpu().numpy()

    gi = run(DEV)
    oi = _with_oracle(lambda: run("cpu"))
    assert gi.shape == (3, 3, *hw) and all(gi[v].max() > 0.05 for v in range(3)) and rel_l2(gi, oi) < parity_checks.TOL


def _compare_extrinsics_grad(got, want):
    """The whole of extrinsics.grad per view: rotation block, translation column and bottom row each rel-L2 < TOL.  (The bottom row is
    not zero: the records hold inverse(extrinsics), and the gradient of a matrix inverse, -A^T dA A^T, fills it - as autograd through
    the reference's `extrinsics.inverse()` does; both sides must agree on it like on the rest.)"""
    got, want = got.reshape(-1, 4, 4), want.reshape(-1, 4, 4)
    assert got.shape == want.shape and np.isfinite(got).all()
    for v in range(got.shape[0]):
        assert np.abs(want[v, :3, :3]).min() > 0 and np.abs(want[v, :3, 3]).min() > 0, v
        assert rel_l2(got[v, :3, :3], want[v, :3, :3]) < parity_checks.TOL, (v, "rotation", got[v], want[v])
        assert rel_l2(got[v, :3, 3], want[v, :3, 3]) < parity_checks.TOL, (v, "translation", got[v], want[v])
        assert rel_l2(got[v, 3], want[v, 3]) < parity_checks.TOL, (v, "bottom row", got[v], want[v])


@pytest.mark.parametrize("camera_gradient", ["full", "depth"])
def test_decoder_pose_gradients_match_the_oracle_driven_decoder(camera_gradient):
    """DecoderSplattingCUDA.forward(depth_mode="depth") on three rolled cameras: pose_gradients=True (every term reaches `extrinsics`) and
    the default with `extrinsics` requiring grad (the reference graph's one term, through the depth channel)."""
    sc = case("d_full").scenes[0]
    hw = sc.image_shape
    g = torch.Generator().manual_seed(3)
    w, wd = torch.rand((1, 3, 3, *hw), generator=g), torch.rand((1, 3, *hw), generator=g)

    def run(device):
        dec = pf3plat_amd.DecoderSplattingCUDA(dataset_cfg=pf3plat_amd.decoder.DatasetCfgLike((0.2, 0.1, 0.0)), on_overflow=None).to(device)
        m, c, h, o = _leafs(sc, device)
        ext = sc.extrinsics.clone().to(device).requires_grad_(True)
        out = dec.forward(Gaussians(m, c, h, o), ext, sc.intrinsics.to(device), sc.near.to(device), sc.far.to(device), hw, depth_mode="depth",
                          pose_gradients=camera_gradient == "full")
        ((out.color * w.to(device)).sum() + (out.depth * wd.to(device)).sum()).backward()
        return out.color.detach().cpu().numpy(), out.depth.detach().cpu().numpy(), (m, c, h, o), ext.grad.cpu().numpy()

    gc, gd, gl, ge = run(DEV)
    oc, od, ol, oe = _with_oracle(lambda: run("cpu"))
    assert rel_l2(gc, oc) < parity_checks.TOL and rel_l2(gd, od) < parity_checks.TOL
    _same_grads(gl, ol)
    _compare_extrinsics_grad(ge, oe)
