"""GSR_FLAG_SH_IN_FRAME on the MI355X: the kernels evaluate harmonics given in their group's frame at the view direction carried
into it.  Every case is compared with the path it replaces - the coefficients rotated by `sh_rotation.rotate_sh` in torch, then the
HIP path as it was: images, dL/d(frame harmonics) (autograd through rotate_sh), dL/dmeans, dL/d(scale, quaternion), dL/dopacities,
camera gradients; and end to end, the fused adapter against the default one through the decoder."""
import numpy as np
import pytest
import torch

import pf3plat_amd
from pf3plat_amd import _lib, rasterizer, synthetic
from pf3plat_amd.adapter import GaussianAdapter, GaussianAdapterCfg
from pf3plat_amd.rasterizer import RasterConfig, _rotate_in_frames
from pf3plat_amd.sh_rotation import rotate_sh
from pf3plat_amd.types import Gaussians
from tests import gpu_util
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BITS = {"rasterizer": _lib.FLAG_SH_IN_FRAME, "e3nn": _lib.FLAG_SH_IN_FRAME | _lib.FLAG_SH_FRAME_E3NN}
DEPTH = 1 << 4  # GSR_FLAG_EXTRA_MODE(GSR_EXTRA_DEPTH)


def _frames(f, seed):
    q = torch.linalg.qr(torch.randn(1, f, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)))[0]
    return (q * torch.det(q)[..., None, None]).float()  # proper rotations


def _inputs(n, views, hw, m, planar, f, seed):
    sc = synthetic.make_scene(seed, n, hw, num_views=views)
    g = torch.Generator().manual_seed(seed + 1)
    means = sc.gaussians.means.contiguous()
    depth = means[0].norm(dim=-1)
    scales = (0.5 + 14.5 * torch.rand((1, n, 3), generator=g)) * depth[None, :, None] * (4.0 / (0.86 * hw[1]))
    records = torch.cat((scales, torch.randn((1, n, 4), generator=g)), -1)
    opac = (0.2 + 0.7 * torch.rand((1, n), generator=g))
    sh = 0.4 * torch.randn((1, n, 3, m) if planar else (1, n, m, 3), generator=g)
    vb = gpu_util.scene_viewbuf(sc)
    return [x.to(DEV) for x in (means, records, opac, sh, vb, _frames(f, seed + 2))]


def _world(sh, frames, planar, basis):
    return _rotate_in_frames(sh.double(), frames.double(), planar, basis).float().contiguous()


def _cfg(views, n, hw, deg, m, mse, flags):
    return RasterConfig(views, 1, views, n, hw[0], hw[1], deg, m, mse, True, flags | DEPTH, True)


@pytest.mark.parametrize("basis", ["e3nn", "rasterizer"])
@pytest.mark.parametrize("path", ["colour_in_binning", "k_color", "windowed"])
def test_fused_forward_equals_rotate_sh_then_render(basis, path):
    hip = rasterizer.HipBackend()
    views, flags = {"colour_in_binning": (2, 0), "k_color": (8, 0), "windowed": (2, _lib.FLAG_WINDOWED_BINNING)}[path]
    n, hw = 640, (64, 64)
    d = hip._dims(_cfg(views, n, hw, 4, 25, 4, flags), 1 << 16)
    assert hip.lib.gsr_colour_in_binning(d) == (1 if path == "colour_in_binning" else 0)
    checked = 0
    for deg, m, mse in ((1, 4, 4), (2, 9, 4), (3, 16, 4), (4, 25, 4), (2, 25, 4), (4, 25, 3)):
        for planar in (True, False):
            for f in (1, 2, 4):  # 4: groups of 160 Gaussians, so units of 64 straddle two frames
                means, records, opac, sh, vb, fr = _inputs(n, views, hw, m, planar, f, seed=deg * 10 + f)
                base = flags | (_lib.FLAG_SH_PLANAR if planar else 0)
                c, e, _, _ = hip.forward(_cfg(views, n, hw, deg, m, mse, base | BITS[basis]), vb, means, records, opac, sh, None, frames=fr)
                cfg = _cfg(views, n, hw, deg, m, mse, base)
                rc, re_, _, _ = hip.forward(cfg, vb, means, records, opac, _world(sh, fr, planar, basis), None, frames=fr)
                plain, _, _, _ = hip.forward(cfg, vb, means, records, opac, sh, None, frames=fr)
                c, rc, plain = c.cpu().numpy(), rc.cpu().numpy(), plain.cpu().numpy()
                case = (deg, m, mse, planar, f)
                assert np.abs(rc).max() > 0.05, case
                assert rel_l2(c, rc) <= 1e-5, case
                assert rel_l2(e.cpu().numpy(), re_.cpu().numpy()) <= 1e-6, case
                assert rel_l2(plain, rc) > 1e-2, case  # a kernel that ignored the bit would render `plain`
                checked += 1
    assert checked == 36


def _grads(hip, cfg, vb, means, records, opac, sh, fr, gc, ge, follows, want_views=False):
    c, e, _, saved = hip.forward(cfg, vb, means, records, opac, sh, None, frames=fr)
    g = hip.backward(cfg, saved, vb, means, records, opac, sh, None, gc, ge, False, rows_in_workspace=follows, frames=fr,
                     want_views=want_views)
    return c, g


@pytest.mark.parametrize("basis", ["e3nn", "rasterizer"])
@pytest.mark.parametrize("follows", [False, True])
@pytest.mark.parametrize("views", [1, 3])
def test_fused_backward_equals_autograd_through_rotate_sh(basis, follows, views):
    """dL/d(frame harmonics), dL/dmeans, dL/d(scale, quaternion), dL/dopacities: one walk (Vs = 1) and the second walk (Vs = 3
    without a saved Jacobian), with and without the saved Jacobian (GSR_FLAG_BACKWARD_FOLLOWS); F = 4 groups that straddle units."""
    hip = rasterizer.HipBackend()
    n, hw = 640, (64, 64)
    means, records, opac, sh, vb, fr = _inputs(n, views, hw, 25, True, 4, seed=70 + views)
    g = torch.Generator().manual_seed(5)
    gc = torch.rand((views, 3, *hw), generator=g).to(DEV)
    ge = (0.05 * torch.rand((views, *hw), generator=g)).to(DEV)
    base = _lib.FLAG_SH_PLANAR | (_lib.FLAG_BACKWARD_FOLLOWS if follows else 0)
    cfg_f = _cfg(views, n, hw, 4, 25, 4, base | BITS[basis])
    cfg_r = _cfg(views, n, hw, 4, 25, 4, base)
    _, gf = _grads(hip, cfg_f, vb, means, records, opac, sh, fr, gc, ge, follows)
    local = sh.detach().double().requires_grad_(True)
    world = _rotate_in_frames(local, fr.double(), True, basis)
    _, gr = _grads(hip, cfg_r, vb, means, records, opac, world.detach().float().contiguous(), fr, gc, ge, follows)
    d_local = torch.autograd.grad(world, local, gr[3].double())[0]
    for k, name, want in ((0, "means", gr[0]), (1, "scale_rot", gr[1]), (2, "opacities", gr[2]), (3, "harmonics", d_local)):
        assert want.abs().max() > 0, name
        assert rel_l2(gf[k].cpu().numpy(), want.cpu().numpy()) <= 1e-4, name


def test_fused_backward_is_deterministic_and_carries_camera_gradients():
    """GSR_FLAG_DETERMINISTIC: two runs give the same bits.  Camera gradients (all of them, and the depth channel's term alone)
    equal the unfused path's: the direction gradient reaches the camera centre in world coordinates."""
    hip = rasterizer.HipBackend()
    n, hw, views = 640, (64, 64), 3
    means, records, opac, sh, vb, fr = _inputs(n, views, hw, 25, True, 4, seed=90)
    g = torch.Generator().manual_seed(6)
    gc = torch.rand((views, 3, *hw), generator=g).to(DEV)
    ge = (0.05 * torch.rand((views, *hw), generator=g)).to(DEV)
    for follows in (False, True):
        base = _lib.FLAG_SH_PLANAR | _lib.FLAG_DETERMINISTIC | (_lib.FLAG_BACKWARD_FOLLOWS if follows else 0)
        cfg = _cfg(views, n, hw, 4, 25, 4, base | BITS["e3nn"])
        runs = [_grads(hip, cfg, vb, means, records, opac, sh, fr, gc, ge, follows)[1] for _ in range(2)]
        for a, b in zip(runs[0][:4], runs[1][:4]):
            assert torch.equal(a, b)
        world = _world(sh, fr, True, "e3nn")
        for want_views in (True, "depth"):
            _, gf = _grads(hip, cfg, vb, means, records, opac, sh, fr, gc, ge, follows, want_views=want_views)
            _, gr = _grads(hip, _cfg(views, n, hw, 4, 25, 4, base), vb, means, records, opac, world, fr, gc, ge, follows,
                           want_views=want_views)
            assert gr[6].abs().max() > 0
            assert rel_l2(gf[6].cpu().numpy(), gr[6].cpu().numpy()) <= 1e-4, want_views
            assert rel_l2(gf[0].cpu().numpy(), gr[0].cpu().numpy()) <= 1e-4, want_views


def _adapter_inputs(seed=11, hs=256, ws=256, b=1):
    """Two source cameras per scene (x = -0.5 / +0.5, turned by a few degrees - proper, non-trivial frames; scene k > 0 turned a little
    further, so that every scene has frames of its own), one Gaussian per pixel of each.  b scenes."""
    g = torch.Generator().manual_seed(seed)
    ext = torch.eye(4).repeat(b, 2, 1, 1)
    for k in range(b):
        for v, (x, ang) in enumerate(((-0.5, 0.12), (0.5, -0.09))):
            ang += 0.07 * k
            c, s = np.cos(ang), np.sin(ang)
            ext[k, v, :3, :3] = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float32) @ \
                torch.tensor([[1, 0, 0], [0, np.cos(0.05), -np.sin(0.05)], [0, np.sin(0.05), np.cos(0.05)]], dtype=torch.float32)
            ext[k, v, 0, 3] = x
    intr = torch.tensor([[0.86, 0, 0.5], [0, 0.86, 0.5], [0, 0, 1]]).repeat(b, 2, 1, 1)
    yy, xx = torch.meshgrid((torch.arange(hs) + 0.5) / hs, (torch.arange(ws) + 0.5) / ws, indexing="ij")
    coords = torch.stack((xx, yy), -1).reshape(1, 1, hs * ws, 2).expand(b, 2, hs * ws, 2)
    depths = 3.0 + torch.sin(6 * xx + 2 * yy).reshape(1, 1, hs * ws) + 0.02 * torch.rand((b, 2, hs * ws), generator=g)
    opac = 0.1 + 0.85 * torch.rand((b, 2, hs * ws), generator=g)
    raw = torch.randn((b, 2, hs * ws, 82), generator=g)
    return ext, intr, coords, depths, opac, raw


@pytest.mark.parametrize("basis", ["e3nn", "rasterizer"])
def test_fused_adapter_end_to_end_at_pf3plat_size(basis):
    """2 source views x 256^2 pixel-aligned Gaussians, 3 target views, colour + depth through DecoderSplattingCUDA: the fused adapter
    (harmonics in the source camera's frame, rotated in the kernels) against the default adapter (rotate_sh in torch)."""
    ext, intr, coords, depths, opac, raw0 = _adapter_inputs()  # (the adapter runs on the CPU; its outputs move to the device)
    sc = synthetic.make_scene(50, 8, (256, 256), num_views=3)
    cams = [x.to(DEV) for x in (sc.extrinsics, sc.intrinsics, sc.near, sc.far)]
    g = torch.Generator().manual_seed(7)
    w = torch.rand((1, 3, 3, 256, 256), generator=g).to(DEV)
    wd = (0.05 * torch.rand((1, 3, 256, 256), generator=g)).to(DEV)
    dec = pf3plat_amd.DecoderSplattingCUDA().to(DEV)
    cfg = GaussianAdapterCfg(0.5, 15.0, 4)
    res = []
    for fused in (True, False):
        ad = GaussianAdapter(cfg, fuse_sh_rotation=True, sh_basis=basis) if fused else \
            GaussianAdapter(cfg, rotate_sh=lambda s, r: rotate_sh(s, r, basis=basis))
        raw = raw0.clone().requires_grad_(True)
        out = ad.forward(ext[:, :, None], intr[:, :, None], coords, depths, opac, raw, (256, 256))
        gs = out.for_decoder()
        mv = lambda x: None if x is None else x.to(DEV)
        gs = Gaussians(mv(gs.means), None, mv(gs.harmonics), mv(gs.opacities), mv(gs.scales), mv(gs.rotations), mv(gs.frames), gs.sh_frame)
        assert gs.sh_frame == (basis if fused else None) and gs.means.shape == (1, 131072, 3)
        o = dec.forward(gs, *cams, (256, 256), depth_mode="depth")
        ((o.color * w).sum() + (o.depth * wd).sum()).backward()
        res.append((o.color.detach().cpu().numpy(), o.depth.detach().cpu().numpy(), raw.grad.cpu().numpy()))
    assert np.abs(res[1][0]).max() > 0.1 and np.abs(res[1][2][..., 7:]).max() > 0
    assert rel_l2(res[0][0], res[1][0]) <= 1e-5 and rel_l2(res[0][1], res[1][1]) <= 1e-5
    assert rel_l2(res[0][2], res[1][2]) <= 1e-4
