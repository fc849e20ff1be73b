"""The extended launch entry points (gsr_forward_ex / gsr_backward_ex) through the plan API on the MI355X: stage timing
(`profile=True`) in the scale / rotation form and together with camera gradients returns the bits of the untimed call, and NULL options
are the plain gsr_forward; and all four options of a launch - scale / rotation form, stage timing, camera gradients, accumulated alpha
- meet in one struct each way.  One small shape: 1 set x 2 views of 16 x 16 pixels, 128 Gaussians, degree 4 (25 coefficients) in
F = 2 frames ("rasterizer" basis), built-in depth channel, a forward that announces its backward - the frame instances of the
colour pass, the saved Jacobian and both backward kernels."""
import numpy as np
import pytest
import torch

from pf3plat_amd import _lib, rasterizer, synthetic
from pf3plat_amd.rasterizer import RasterConfig
from tests import gpu_util

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DEPTH = 1 << 4  # GSR_FLAG_EXTRA_MODE(GSR_EXTRA_DEPTH)
N, HW, VIEWS = 128, (16, 16), 2
OUTPUTS = ("color", "extra_img", "radii")
GRADS = ("d_means", "d_cov6", "d_opac", "d_colors", "d_extra", "d_means2d")


@pytest.fixture(scope="module")
def case():
    sc = synthetic.make_scene(150, N, HW, num_views=VIEWS, d_sh=1)
    g = torch.Generator().manual_seed(150)
    means, opac = sc.gaussians.means.contiguous(), sc.gaussians.opacities.contiguous()
    scales = (0.5 + 14.5 * torch.rand((1, N, 3), generator=g)) * means.norm(dim=-1, keepdim=True) * (4.0 / (0.86 * HW[1]))
    records = torch.cat((scales, torch.randn((1, N, 4), generator=g)), -1)
    sh = 0.4 * torch.randn((1, N, 3, 25), generator=g)
    q = torch.linalg.qr(torch.randn((1, 2, 3, 3), dtype=torch.float64, generator=g))[0]
    frames = (q * torch.det(q)[..., None, None]).float()
    cov6 = gpu_util.cov6_in_kernel_order(records, frames)
    gc, ge = torch.rand((VIEWS, 3, *HW), generator=g), torch.rand((VIEWS, *HW), generator=g)
    vb = gpu_util.scene_viewbuf(sc)
    return {k: v.to(DEV).contiguous() for k, v in dict(vb=vb, means=means, records=records, cov6=cov6, opac=opac, sh=sh, frames=frames,
                                                       gc=gc, ge=ge).items()}


def _sr_plan(hip):
    flags = DEPTH | _lib.FLAG_DETERMINISTIC | _lib.FLAG_SH_PLANAR | _lib.FLAG_BACKWARD_FOLLOWS | gpu_util.SH_FRAME_BITS["rasterizer"]
    return hip.make_plan(RasterConfig(VIEWS, 1, VIEWS, N, *HW, 4, 25, 4, True, flags, True), DEV, 1 << 16, backward=True)


def _step(hip, plan, c, profile, d_views=None):
    """One forward + backward on the plan -> (stage ms of each or None, copies of every output, the status block)."""
    plan["d_extra"].zero_()  # (not written with the built-in channel: defined, so that it can be compared)
    fwd_ms = hip.run_forward(plan, c["vb"], c["means"], c["records"], c["opac"], c["sh"], None, profile=profile, frames=c["frames"])
    bwd_ms = hip.run_backward(plan, c["vb"], c["means"], c["records"], c["opac"], c["sh"], None, c["gc"], c["ge"], profile=profile,
                              frames=c["frames"], d_views=d_views)
    torch.cuda.synchronize()
    return fwd_ms, bwd_ms, {k: plan[k].clone() for k in OUTPUTS + GRADS}, hip.read_status(plan)


@pytest.fixture(scope="module")
def unprofiled(case):
    hip = rasterizer.HipBackend()
    fwd_ms, bwd_ms, out, status = _step(hip, _sr_plan(hip), case, False)
    assert fwd_ms is None and bwd_ms is None and not status["overflow"] and status["num_pairs"] > 0
    assert int((out["radii"] > 0).sum()) >= N // 4 and float(out["extra_img"].max()) > 0
    for k in ("d_means", "d_cov6", "d_opac", "d_colors", "d_means2d"):
        assert float(out[k].abs().max()) > 0, k
    assert float(out["d_colors"][..., 1:].abs().max()) > 0  # (the bands above DC: the harmonics in their frames are evaluated)
    return out


def test_profile_in_the_scale_rotation_form_returns_stage_times_and_the_same_bits(case, unprofiled):
    hip = rasterizer.HipBackend()
    fwd_ms, bwd_ms, out, status = _step(hip, _sr_plan(hip), case, True)
    assert not status["overflow"]
    for ms, stages in ((fwd_ms, _lib.FWD_STAGES), (bwd_ms, _lib.BWD_STAGES)):
        assert tuple(ms) == stages
        assert all(np.isfinite(x) and x >= 0 for x in ms.values()), ms
    assert fwd_ms["tiles"] > 0 and bwd_ms["blend_bwd"] > 0 and bwd_ms["preprocess_bwd"] > 0
    for k in OUTPUTS + GRADS:
        assert torch.equal(out[k], unprofiled[k]), k


def test_profile_together_with_camera_gradients_returns_the_same_bits(case, unprofiled):
    hip = rasterizer.HipBackend()
    d_views = [torch.full((VIEWS, rasterizer.VIEW_FLOATS), float("nan"), device=DEV) for _ in range(2)]
    plan = _sr_plan(hip)
    _, plain_ms, plain, _ = _step(hip, plan, case, False, d_views[0])
    _, bwd_ms, timed, _ = _step(hip, plan, case, True, d_views[1])
    assert plain_ms is None and tuple(bwd_ms) == _lib.BWD_STAGES and all(np.isfinite(x) and x >= 0 for x in bwd_ms.values())
    assert bool(torch.isfinite(d_views[0]).all()) and float(d_views[0].abs().max()) > 0
    assert torch.equal(d_views[1], d_views[0])
    for k in OUTPUTS + GRADS:
        assert torch.equal(timed[k], plain[k]) and torch.equal(timed[k], unprofiled[k]), k


def test_all_four_options_in_one_struct_each_way(case, unprofiled):
    """Scale / rotation form with frames, stage timing, camera gradients and the accumulated alpha with its cotangent in the same
    GsrForwardOptions / GsrBackwardOptions: the timed step returns the bits of the untimed one, and the cotangent arrives."""
    hip = rasterizer.HipBackend()
    flags = DEPTH | _lib.FLAG_DETERMINISTIC | _lib.FLAG_SH_PLANAR | _lib.FLAG_BACKWARD_FOLLOWS | gpu_util.SH_FRAME_BITS["rasterizer"]
    plan = hip.make_plan(RasterConfig(VIEWS, 1, VIEWS, N, *HW, 4, 25, 4, True, flags, True, True), DEV, 1 << 16, backward=True)
    assert plan["alpha_img"].shape == (VIEWS, *HW)
    c = case
    g_alpha = torch.rand((VIEWS, *HW), generator=torch.Generator().manual_seed(151)).to(DEV)
    runs = []
    for profile in (False, True):
        d_views = torch.full((VIEWS, rasterizer.VIEW_FLOATS), float("nan"), device=DEV)
        plan["d_extra"].zero_()  # (not written with the built-in channel)
        plan["alpha_img"].fill_(float("nan"))
        fwd_ms = hip.run_forward(plan, c["vb"], c["means"], c["records"], c["opac"], c["sh"], None, profile=profile, frames=c["frames"])
        bwd_ms = hip.run_backward(plan, c["vb"], c["means"], c["records"], c["opac"], c["sh"], None, c["gc"], c["ge"], profile=profile,
                                  frames=c["frames"], d_views=d_views, g_alpha_img=g_alpha)
        torch.cuda.synchronize()
        assert not hip.read_status(plan)["overflow"]
        runs.append((fwd_ms, bwd_ms, dict({k: plan[k].clone() for k in OUTPUTS + GRADS + ("alpha_img",)}, d_views=d_views)))
    (plain_fwd, plain_bwd, plain), (fwd_ms, bwd_ms, timed) = runs
    assert plain_fwd is None and plain_bwd is None and tuple(fwd_ms) == _lib.FWD_STAGES and tuple(bwd_ms) == _lib.BWD_STAGES
    assert all(np.isfinite(x) and x >= 0 for ms in (fwd_ms, bwd_ms) for x in ms.values())
    for k in plain:
        assert torch.equal(timed[k], plain[k]), k
    alpha = plain["alpha_img"]
    assert bool(torch.isfinite(alpha).all()) and float(alpha.min()) >= 0 and float(alpha.max()) < 1 and float(alpha.max()) > 0
    assert bool(torch.isfinite(plain["d_views"]).all()) and float(plain["d_views"].abs().max()) > 0
    assert not torch.equal(plain["d_opac"], unprofiled["d_opac"])  # (`unprofiled` has no alpha cotangent: this one came through the struct)


def test_null_options_are_the_plain_forward(case):
    """gsr_forward_ex with NULL options (run_forward on a plain plan) against gsr_forward (bind_forward), covariance form."""
    hip = rasterizer.HipBackend()
    c = case
    plan = hip.make_plan(RasterConfig(VIEWS, 1, VIEWS, N, *HW, 4, 25, 4, True, DEPTH | _lib.FLAG_SH_PLANAR), DEV, 1 << 16)
    args = (plan, c["vb"], c["means"], c["cov6"], c["opac"], c["sh"], None)
    assert hip.run_forward(*args) is None
    torch.cuda.synchronize()
    assert not hip.read_status(plan)["overflow"]
    ex = {k: plan[k].clone() for k in OUTPUTS}
    for k in OUTPUTS:
        plan[k].zero_()
    hip.bind_forward(*args)()
    torch.cuda.synchronize()
    assert int((ex["radii"] > 0).sum()) >= N // 4 and float(ex["extra_img"].max()) > 0
    for k in OUTPUTS:
        assert torch.equal(plan[k], ex[k]), k
