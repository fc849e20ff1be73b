"""Learnable intrinsics on the MI355X: the tan-fov columns of the camera gradient (GSR_FLAG_FOV_GRADIENT, floats 35 and 36 of a
record's row), the 37-column reduce, gsr_setup_views_backward_ex and the torch surface (`intrinsics_gradients=True`).

The tan-fov gradient has no analytic oracle, so the reference is the central finite difference of the fp64 oracle's forward over the two
scalars (tests/fov_rig.py), on a camera-rig case that tests/test_fov_gradient.py holds to its guard on the CPU: seed guard, a clamped
Gaussian in every view, differences that agree between two steps to 2e-6.  The bound is not a constant: the same run's other camera
columns are measured against the fp64 oracle's analytic gradient (d_ref), and the new columns may sit twice that far from the
differences, plus two finite-difference errors - capped at the project's fp32-against-fp64 camera bar, 2e-4.  docs/PARITY.md section 10
has the measured figures and the two mutations the record-level test was run against."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import pf3plat_amd
from pf3plat_amd import _lib, rasterizer
from pf3plat_amd.types import Gaussians
from tests import camera_rig, fov_rig, gpu_util, parity_checks
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FOLLOWS, DET, FOV = _lib.FLAG_BACKWARD_FOLLOWS, _lib.FLAG_DETERMINISTIC, _lib.FLAG_FOV_GRADIENT
BLOCKS = ((0, 16), (16, 32), (32, 35))
CAP = 2e-4  # fp32 against fp64 on a camera gradient (tests/test_oracle_pose_grad.py): no d_ref lifts the bound above it


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _hip(c, flags=0):
    ch = c.with_flags(flags)
    return gpu_util.run_hip(ch.cfg, c.vb, c.means, c.cov, c.opac, c.colors, c.extra, c.gc, c.ge, frames=c.frames, sh_frame=c.sh_frame,
                            want_views=c.want_views)


@functools.lru_cache(maxsize=None)
def _analytic64():
    """The fp64 oracle's analytic camera gradient (V, 48) of the guarded case: computed once, left unchanged."""
    c = fov_rig.guarded_case()
    g = gpu_util.run_oracle(*c.args(), c.gc, c.ge, np.float64, True, True)["grads"]["views"]
    g.setflags(write=False)
    return g


def _d_ref(views):
    """Worst over views and blocks of max|hip - o64| / max|o64|: how far the kernel's existing camera columns sit from fp64."""
    o64 = _analytic64()
    return max(float(np.abs(views[v, lo:hi] - o64[v, lo:hi]).max() / np.abs(o64[v, lo:hi]).max())
               for v in range(views.shape[0]) for lo, hi in BLOCKS)


def _bound(d_ref):
    return min(2.0 * d_ref + 4e-6, CAP)


def _check_35(views):
    """check_camera_grads for [0, 35) (it requires zeros behind: the two new columns are cleared in a copy)."""
    h = views.copy()
    h[:, 35:37] = 0.0
    return parity_checks.check_camera_grads(dict(hip=dict(grads=dict(views=h)), oracle=dict(grads=dict(views=_analytic64()))))


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("follows", [False, True])
def test_tanfov_gradient_against_fp64_differences(follows, det):
    c = fov_rig.guarded_case()
    flags = FOV | (FOLLOWS if follows else 0) | (DET if det else 0)
    views = _hip(c, flags)["grads"]["views"].astype(np.float64)
    fd = fov_rig.reference()[0]
    d_ref = _d_ref(views)
    err = [float(np.abs(views[v, 35:37] - fd[v]).max() / np.abs(fd[v]).max()) for v in range(views.shape[0])]
    print(f"follows={follows} det={det} d_ref={d_ref:.3e} err_v={[f'{e:.3e}' for e in err]} bound={_bound(d_ref):.3e} hip={views[:, 35:37].tolist()}")
    assert all(e <= _bound(d_ref) for e in err), (err, d_ref)
    assert _check_35(views) < parity_checks.TOL
    assert not views[:, 37:].any()
    assert (views[:, 35] != 0).all() and (views[:, 36] != 0).all()


def test_without_the_flag_the_slots_stay_zero():
    c = fov_rig.guarded_case()
    views = _hip(c, 0)["grads"]["views"]
    assert np.abs(views[:, :35]).max() > 0 and not _bits(views[:, 35:]).any()


def test_the_flag_touches_nothing_else():
    c = fov_rig.guarded_case()
    off, on, again = _hip(c, DET), _hip(c, DET | FOV), _hip(c, DET | FOV)
    for name in ("color", "extra", "radii"):
        assert np.array_equal(off[name], on[name]), name
    for name in ("means", "cov6", "opac", "colors", "means2d"):
        assert np.array_equal(_bits(off["grads"][name]), _bits(on["grads"][name])), name
    a, b = off["grads"]["views"], on["grads"]["views"]
    for v in range(a.shape[0]):
        for lo, hi in BLOCKS:  # (the 37-wide reduce adds the same rows in another order)
            assert np.abs(a[v, lo:hi] - b[v, lo:hi]).max() <= 1e-5 * np.abs(a[v, lo:hi]).max(), (v, lo)
    assert np.array_equal(_bits(b), _bits(again["grads"]["views"]))
    for name in ("means", "cov6", "opac", "colors", "means2d"):
        assert np.array_equal(_bits(on["grads"][name]), _bits(again["grads"][name])), name


def test_the_depth_term_alone_ignores_the_flag():
    """depth_term_only returns the z row only: with the flag, the same bits and nothing in the tan-fov slots."""
    c = dataclasses.replace(fov_rig.guarded_case(), want_views="depth")
    off, on = _hip(c, DET)["grads"]["views"], _hip(c, DET | FOV)["grads"]["views"]
    assert np.abs(off[:, [2, 6, 10, 14]]).min() > 0 and np.array_equal(_bits(off), _bits(on)) and not _bits(on[:, 16:]).any()


@pytest.mark.parametrize("n", [37, 64, 65, 131072 + 37])
def test_reduce_of_37_columns_at_its_size_edges(n):
    """One view, 64 x 64, colour only; the oracle's analytic [0, 35) is the reference.  37: a partial wave; 64, 65: one and two
    workgroups (fewer rows than reducing blocks); 131 109: 8 196 rows, 33 per block of level 1 - its four-loads-in-flight loop and its
    tail.  A wrong stride or row count in the 37-column instance breaks these columns as well."""
    c = camera_rig.rig_case(seed=900, n=n, hw=(64, 64), views=1, extra=None, want_views=True).with_flags(FOV)
    res = gpu_util.run_both(c.cfg, c.vb, c.means, c.cov, c.opac, c.colors, c.extra, c.gc, c.ge, want_views=True)
    assert not res["hip"]["status"]["overflow"]
    views = res["hip"]["grads"]["views"]
    assert views[0, 35] != 0 and views[0, 36] != 0 and not views[:, 37:].any()
    h = views.copy()
    h[:, 35:37] = 0.0
    worst = parity_checks.check_camera_grads(dict(hip=dict(grads=dict(views=h)), oracle=res["oracle"]))
    assert 0 < worst < parity_checks.TOL


# ---- the set-up chain -----------------------------------------------------------------------------------------------------------------
def _cameras(v, seed):
    g = torch.Generator().manual_seed(seed)
    ext = torch.eye(4).repeat(v, 1, 1)
    q = torch.linalg.qr(torch.randn((v, 3, 3), generator=g, dtype=torch.float64))[0]
    ext[:, :3, :3] = (q * torch.det(q)[:, None, None]).float()
    ext[:, :3, 3] = torch.randn((v, 3), generator=g)
    intr = torch.eye(3).repeat(v, 1, 1)
    j = 0.1 * (torch.rand((v, 4), generator=g) - 0.5)
    intr[:, 0, 0], intr[:, 1, 1], intr[:, 0, 2], intr[:, 1, 2] = 0.8 + j[:, 0], 0.9 + j[:, 1], 0.47 + j[:, 2], 0.55 + j[:, 3]
    near = 0.5 + torch.rand(v, generator=g)
    return ext, intr, near, torch.full((v,), 100.0), g


@pytest.mark.parametrize("scale_invariant", [True, False])
@pytest.mark.parametrize("v", [1, 64, 65])
def test_setup_views_backward_ex_against_float64_autograd(v, scale_invariant):
    be = rasterizer.get_backend()
    ext, intr, near, far, g = _cameras(v, 7 + v)
    vb = be.setup_views(ext.to(DEV), intr.to(DEV), near.to(DEV), far.to(DEV), torch.zeros(3, device=DEV), scale_invariant)
    dvw = torch.randn((v, 48), generator=g)
    dvw[:, 37:] = 0.0
    d_ext, d_intr = be.setup_views_backward_ex(vb, intr.to(DEV), dvw.to(DEV))
    k = intr.double().requires_grad_(True)  # the same fp32 intrinsics and the same fp32 record: input rounding does not enter
    fov_rig.record_loss64(vb.cpu(), k, dvw).backward()
    got, want = d_intr.cpu().double().numpy(), k.grad.numpy()
    assert got.shape == (v, 3, 3) and np.abs(want).max() > 0
    assert rel_l2(got, want) < 1e-6
    assert max(rel_l2(got[i], want[i]) for i in range(v)) < 1e-6
    assert np.array_equal(_bits(d_ext.cpu().numpy()), _bits(be.setup_views_backward(vb, dvw.to(DEV)).cpu().numpy()))
    only_intr = be.setup_views_backward_ex(vb, intr.to(DEV), dvw.to(DEV), want_extrinsics=False)
    assert only_intr[0] is None and np.array_equal(_bits(only_intr[1].cpu().numpy()), _bits(d_intr.cpu().numpy()))


# ---- the torch surface ----------------------------------------------------------------------------------------------------------------
def _decode(c, intrinsics_gradients, pose_gradients=False):
    sc = c.scenes[0]
    hw = sc.image_shape
    dec = pf3plat_amd.DecoderSplattingCUDA(dataset_cfg=pf3plat_amd.decoder.DatasetCfgLike(tuple(sc.background.tolist())), on_overflow=None).to(DEV)
    gs = sc.gaussians
    leafs = [t.detach().clone().to(DEV).requires_grad_(True) for t in (gs.means, gs.covariances, gs.harmonics, gs.opacities)]
    ext = sc.extrinsics.clone().to(DEV).requires_grad_(True)
    intr = sc.intrinsics.clone().to(DEV).requires_grad_(True)
    kw = dict(intrinsics_gradients=True) if intrinsics_gradients else {}
    out = dec.forward(Gaussians(*leafs), ext, intr, sc.near.to(DEV), sc.far.to(DEV), hw, depth_mode="depth", pose_gradients=pose_gradients, **kw)
    assert out.color.shape == (1, 3, 3, *hw) and out.depth.shape == (1, 3, *hw)
    ((out.color[0] * c.gc.to(DEV)).sum() + (out.depth[0] * c.ge.to(DEV)).sum()).backward()
    return ext, intr


def test_decoder_fills_intrinsics_grad_only_when_asked():
    """DecoderSplattingCUDA.forward(depth_mode="depth") on the guarded rig, loss = <gc, colour> + <ge, depth> with the case's fixed random
    weights: fx, fy, cx, cy of `intrinsics.grad` per view against fp64 central differences through the float64 set-up and the fp64
    oracle's forward; the bound is the record-level rule with d_ref of the same case."""
    c = fov_rig.guarded_case()
    sc = c.scenes[0]
    # the float64 set-up restates the product: its records against views_from_cameras' to fp32 rounding
    vb = rasterizer.views_from_cameras(sc.extrinsics[0].to(DEV), sc.intrinsics[0].to(DEV), sc.near[0].to(DEV), sc.far[0].to(DEV),
                                       sc.background.to(DEV)).cpu().double()
    vb64 = fov_rig.setup_views64(sc.extrinsics[0], sc.intrinsics[0].double(), sc.near[0], sc.far[0], sc.background)
    assert float((vb - vb64).abs().max() / vb64.abs().max()) < 1e-6
    for lo, hi in ((0, 16), (16, 32), (32, 35), (35, 37)):
        assert rel_l2(vb[:, lo:hi].numpy(), vb64[:, lo:hi].numpy()) < 1e-6, lo

    ext, intr = _decode(c, False)
    assert intr.grad is None and ext.grad is not None  # today's behaviour: the depth term reaches the extrinsics, nothing the intrinsics
    ext, intr = _decode(c, True)
    assert ext.grad is None and intr.grad is not None and intr.grad.shape == (1, 3, 3, 3)
    rows, cols = zip(*fov_rig.INTRINSICS_ENTRIES)
    got = intr.grad[0][:, rows, cols].cpu().double().numpy()
    fd = fov_rig.intrinsics_reference()[0]
    d_ref = _d_ref(_hip(c, FOV | FOLLOWS)["grads"]["views"].astype(np.float64))
    err = [float(np.abs(got[v] - fd[v]).max() / np.abs(fd[v]).max()) for v in range(3)]
    print(f"d_ref={d_ref:.3e} err_v={[f'{e:.3e}' for e in err]} bound={_bound(d_ref):.3e}")
    assert all(e <= _bound(d_ref) for e in err), (err, d_ref, got, fd)
    others = intr.grad[0].cpu().numpy().copy()
    others[:, rows, cols] = 0.0
    assert np.isfinite(others).all()
    ext, intr = _decode(c, True, pose_gradients=True)
    assert ext.grad is not None and float(ext.grad.abs().max()) > 0 and intr.grad is not None
