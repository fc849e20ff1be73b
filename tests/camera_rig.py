"""General cameras for the parity tests: arbitrary rigid poses that differ from view to view, roll, and have their own anisotropic field
of view and near plane - what a pose-estimation model renders through.  `synthetic.make_scene`'s own cameras have rotation exactly I in
every view, fx = fy and one near per scene; with those the kernels could transpose a view matrix, read view 0's rotation for every view of
a set or swap tan-fov x / y and return the same bits.

`general_cameras(scene, seed)` replaces the cameras of a `make_scene` scene and keeps its Gaussians.  The cases the GPU module
(tests/test_gpu_general_cameras.py) renders are named here (`CASES`), so that the CPU module (tests/test_general_cameras.py) can hold each
of them to the seed guard - fp32 oracle against fp64 oracle through parity_checks with no outlier pixel, no flipped pixel and no row set
aside - and to the properties the rig is for.  Test infrastructure only."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from pf3plat_amd import _lib, synthetic
from pf3plat_amd.rasterizer import RasterConfig
from tests import gpu_util, parity_checks
from tests.util import look_at_c2w

NEARS = (0.5, 1.0, 2.0)


def general_cameras(scene, seed):
    """A pure function of `seed`: per view, in this order from np.random.default_rng(seed): eye, target, roll phi, fx and fy, near.
    The camera looks from `eye` (around the origin, where make_scene's own cameras are) at `target` (inside the cloud) with its up
    vector rolled by phi; far stays 100, the principal point 0.5."""
    rng = np.random.default_rng(seed)
    v = scene.extrinsics.shape[1]
    ext, intr, near = [], [], []
    for _ in range(v):
        eye = rng.uniform([-1.5, -1.5, -2.0], [1.5, 1.5, 0.5])
        target = rng.uniform([-1.0, -1.0, 4.0], [1.0, 1.0, 8.0])
        phi = rng.uniform(-1.0, 1.0)
        ext.append(look_at_c2w(eye, target, up=(np.sin(phi), -np.cos(phi), 0.0)))
        fx, fy = rng.uniform(0.6, 1.3, 2)
        intr.append(np.array([[fx, 0, 0.5], [0, fy, 0.5], [0, 0, 1]], dtype=np.float32))
        near.append(float(rng.choice(NEARS)))
    return dataclasses.replace(scene, extrinsics=torch.tensor(np.stack(ext))[None], intrinsics=torch.tensor(np.stack(intr))[None],
                               near=torch.tensor(near, dtype=torch.float32)[None], far=torch.full((1, v), 100.0))


@dataclasses.dataclass
class Case:
    """One call, CPU tensors: what gpu_util.run_both / run_oracle take.  `scenes`: the rigged scenes (one per set) it was built from."""
    cfg: RasterConfig
    vb: torch.Tensor
    means: torch.Tensor
    cov: torch.Tensor  # (S, N, 6), or (S, N, 7) scale + quaternion records (cfg.scale_rot)
    opac: torch.Tensor
    colors: torch.Tensor
    extra: torch.Tensor | None
    gc: torch.Tensor
    ge: torch.Tensor | None
    frames: torch.Tensor | None = None
    sh_frame: str | None = None
    want_views: object = False
    scenes: tuple = ()

    def args(self):
        return self.cfg, self.vb, self.means, self.cov, self.opac, self.colors, self.extra

    def with_flags(self, flags, **kw):
        return dataclasses.replace(self, cfg=dataclasses.replace(self.cfg, flags=self.cfg.flags | flags), **kw)

    def set_slice(self, s):
        """Set `s` of the call as a single-set call of its own (same tensors, sliced)."""
        vps = self.cfg.views_per_set
        v = slice(s * vps, (s + 1) * vps)
        cfg = dataclasses.replace(self.cfg, num_views=vps, num_sets=1)
        cut = lambda t, k: None if t is None else t[k].contiguous()
        return dataclasses.replace(self, cfg=cfg, vb=self.vb[v], means=cut(self.means, slice(s, s + 1)), cov=cut(self.cov, slice(s, s + 1)),
                                   opac=cut(self.opac, slice(s, s + 1)), colors=cut(self.colors, slice(s, s + 1)), extra=cut(self.extra, v),
                                   gc=self.gc[v], ge=cut(self.ge, v), frames=cut(self.frames, slice(s, s + 1)), scenes=self.scenes[s:s + 1])


def rig_case(seed, n=3000, hw=(64, 80), views=3, sets=1, deg=4, use_sh=True, extra="given", scale_invariant=True, flags=0, want_views=False,
             scale_rot=False, sh_frame=None, alpha=False):
    """make_scene(seed + 1000 s) under general_cameras(., seed + 1000 s) for every set s.  extra: None, "given" (a caller-supplied
    channel) or a built-in mode 1 .. 4 (depth, disparity, relative disparity, log).  scale_rot: (S, N, 7) records in F = 2 frames per set
    (groups of n / 2 Gaussians) and planar harmonics, in those frames' coordinates when `sh_frame` names a basis."""
    h, w = hw
    d_sh = (deg + 1) ** 2
    scs = tuple(general_cameras(synthetic.make_scene(seed + 1000 * s, n, hw, num_views=views, d_sh=1 if scale_rot else d_sh), seed + 1000 * s)
                for s in range(sets))
    vb = torch.cat([gpu_util.scene_viewbuf(sc, scale_invariant) for sc in scs])
    rng = np.random.default_rng(seed)
    v = sets * views
    emode = extra if isinstance(extra, int) else 0
    extra_t = torch.tensor(rng.uniform(0.5, 2.0, (v, n)).astype(np.float32)) if extra == "given" else None
    gc = torch.tensor(rng.uniform(0, 1, (v, 3, h, w)).astype(np.float32))
    ge = torch.tensor(rng.uniform(0, 1, (v, h, w)).astype(np.float32)) if extra is not None else None
    frames = None
    if scale_rot:
        g = torch.Generator().manual_seed(seed)
        means = torch.cat([sc.gaussians.means for sc in scs]).contiguous()
        opac = torch.cat([sc.gaussians.opacities for sc in scs]).contiguous()
        scales = (0.5 + 14.5 * torch.rand((sets, n, 3), generator=g)) * means.norm(dim=-1, keepdim=True) * (4.0 / (0.86 * w))
        cov = torch.cat((scales, torch.randn((sets, n, 4), generator=g)), -1).contiguous()
        colors = 0.4 * torch.randn((sets, n, 3, d_sh), generator=g)
        q = torch.linalg.qr(torch.randn((sets, 2, 3, 3), dtype=torch.float64, generator=g))[0]
        frames = (q * torch.det(q)[..., None, None]).float().contiguous()
        flags |= _lib.FLAG_SH_PLANAR
    else:
        parts = [gpu_util.scene_tensors(sc, use_sh) for sc in scs]
        means, cov, opac, colors = (torch.cat([p[k] for p in parts]).contiguous() for k in range(4))
    cfg = RasterConfig(v, sets, views, n, h, w, deg if use_sh else 0, d_sh if use_sh else 0, 4, extra is not None, (emode << 4) | flags, scale_rot, alpha)
    return Case(cfg, vb, means, cov, opac, colors, extra_t, gc, ge, frames, sh_frame, want_views, scs)


MODES = {"depth": 1, "disparity": 2, "relative_disparity": 3, "log": 4}

# Every case the GPU module renders against the oracle, by name, each with a rig seed of its own.  A seed is the first unused one from
# the case's starting point (a: 101 .., b: 151, c: 201, d: 301, e: 401, f: 501, g: 601, h: 701) upwards that meets
# tests/test_general_cameras.py: the seed guard (with its margin around the alpha threshold) and the rig's properties (among them pairwise
# different near planes within a set, which only two draws in nine of a three-view set have - hence the gaps).
SMALL = dict(n=1000, hw=(45, 70), views=2)
CASES = {
    # a: three views of one set
    "a_sh4_extra": dict(seed=114, deg=4),
    "a_sh0": dict(seed=122, deg=0),
    "a_sh1": dict(seed=181, deg=1),
    "a_sh2": dict(seed=204, deg=2),
    "a_sh3": dict(seed=234, deg=3),
    "a_rgb": dict(seed=235, deg=0, use_sh=False, extra=None),
    # (two views; the first seed from 800 with at least five Gaussians that the z <= 0.2 test culls and a later one with more: 20 in its
    # second view.  The test is the one cull the kernels have - behind the camera or inside the near cull alike; with make_scene's
    # cloud, which starts 0.76 in front of the origin, no seed up to 6000 puts a Gaussian at z <= 0, and one rig in eighty culls any)
    "a_culled": dict(seed=1930, views=2, extra=1, want_views=True),
    # b: several sets, every view with its own camera
    "b_two_sets": dict(seed=156, n=2000, hw=(48, 56), views=2, sets=2, extra=None),
    "b_three_sets": dict(seed=188, n=1500, hw=(48, 56), views=2, sets=3, extra=1, want_views=True),
    # c: the built-in extra modes, with and without the scale-invariant rescale
    **{f"c_{m}_{si}": dict(seed=(208, 209, 210, 213, 218, 220, 223, 224)[2 * k + j], extra=e, scale_invariant=not j, **SMALL)
       for k, (m, e) in enumerate(MODES.items()) for j, si in enumerate(("invariant", "plain"))},
    # d: camera gradients, all of them and the depth channel's term alone
    "d_full": dict(seed=315, extra=1, want_views=True),
    "d_depth": dict(seed=331, extra=1, want_views="depth"),
    # e: scale / rotation records in frames, harmonics in world space or in the frames' coordinates
    "e_None": dict(seed=407, n=600, extra=1, want_views=True, scale_rot=True),
    "e_rasterizer": dict(seed=445, n=600, extra=1, want_views=True, scale_rot=True, sh_frame="rasterizer"),
    "e_e3nn": dict(seed=454, n=600, extra=1, want_views=True, scale_rot=True, sh_frame="e3nn"),
    # f: windowed binning against the fused one
    "f_windowed": dict(seed=503, views=2, extra=None),
    # g: forward instances (colour inside the binning launch, the plain binning launch + colour launch at five views per set)
    "g_colour_in_binning": dict(seed=605, extra=1, **SMALL),
    "g_plain": dict(seed=609, n=1000, hw=(45, 70), views=5, extra=1),
    "g_k_color": dict(seed=606, extra=1, **SMALL),
    # h: accumulated alpha
    "h_alpha": dict(seed=702, extra=1, want_views=True, alpha=True, **SMALL),
}


# fp64 arbitration (test_gpu_general_cameras.py): the largest rel-L2 distance of the fp32 oracle from the fp64 oracle over all the cases
# above that ask for camera gradients, for the one tensor whose bar it becomes (explained there).  Measured with the oracle on ONE
# thread - its plain sequential sum over a view's Gaussians, the same figure on every run: 1.02e-6 at e_rasterizer.  (On eight threads the
# shares are added in the order the threads finish and the figure moves between 2.9e-7 and 4.7e-7 from run to run.)
FP64_FLOOR = {"dL/dviewmatrix": 1.02e-6}


def case(name, **over):
    """Build case `name` (a fresh object every time: tests may not disturb each other's tensors)."""
    return rig_case(**dict(CASES[name], **over))


# ---- the oracle's own rounding on a case: the seed guard, and the middle column of the fp64 arbitration -------------------------------
def oracle_pair(c: Case):
    """-> (fp32 oracle, fp64 oracle) results of gpu_util.run_oracle on the case."""
    run = lambda dt: gpu_util.run_oracle(*c.args(), c.gc, c.ge, dt, True, c.want_views, c.frames, c.sh_frame)
    return run(np.float32), run(np.float64)


def as_hip(o32, cfg):
    """An oracle result in the HIP side's place of a `res` dict: parity_checks reads the saved transmittance from `ws`."""
    return dict(o32, ws=dict(final_T=np.stack([hd[0].image_state()["final_T"] for hd in o32["handles"][:cfg.num_views]])))


ALPHA_MARGIN = 2e-6


def alpha_threshold_margin(c: Case, o32):
    """The closest any (pixel, visible Gaussian) pair of the case comes to the alpha >= 1/255 decision: min |power + log(255 opacity)|
    (= |alpha 255 - 1| to first order) from the fp32 oracle's projected records, evaluated in fp64 at every pixel of every view."""
    h, w = c.cfg.height, c.cfg.width
    px, py = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    px, py = px.reshape(1, -1), py.reshape(1, -1)
    best = np.inf
    for v in range(c.cfg.num_views):
        geo = o32["handles"][v][0].geometry()
        vis = np.asarray(o32["radii"][v]) > 0
        xy, co = geo["xy"][vis].astype(np.float64), geo["conic_opacity"][vis].astype(np.float64)
        for k in range(0, len(xy), 512):
            dx, dy = xy[k:k + 512, 0:1] - px, xy[k:k + 512, 1:2] - py
            power = -0.5 * (co[k:k + 512, 0:1] * dx * dx + co[k:k + 512, 2:3] * dy * dy) - co[k:k + 512, 1:2] * dx * dy
            q = np.abs(power + np.log(255.0 * co[k:k + 512, 3:4]))
            best = min(best, float(q[power <= 0].min(initial=np.inf)))
    return best


def seed_guard(c: Case, o32=None, o64=None):
    """The fp32 oracle in HIP's place against the fp64 oracle through check_image, check_grads and check_camera_grads: 0 outlier pixels,
    0 flipped pixels, nothing set aside.  A condition on the seed, not a measurement: a seed that does not meet it is not used."""
    if o32 is None:
        o32, o64 = oracle_pair(c)
    res = dict(hip=as_hip(o32, c.cfg), oracle=o64)
    mi = parity_checks.check_image(res, c.cfg)
    assert mi["outlier_pixels_1e-4"] == 0 and mi["color_rel_l2_all"] < parity_checks.TOL, mi
    assert mi.get("extra_rel_l2_all", 0.0) < parity_checks.TOL, mi
    mg = parity_checks.check_grads(res, c.cfg)
    assert mg["flipped_pixels"] == 0, mg
    parity_checks.assert_nothing_set_aside(mg)
    worst = parity_checks.check_camera_grads(res) if c.want_views else 0.0
    # and no alpha of the case within fp32 rounding of 1/255: two correct fp32 evaluations of alpha = opacity exp(power) from the SAME
    # record bits differ by the rounding of three products of magnitude up to log(255) = 5.5 (4 x 6e-8 x 5.5 = 1.3e-6), of exp (two
    # ulp, 2.4e-7) and of the last product (6e-8) - under 2e-6.  (Seed 155 of the two-set case: one pair at 2e-7, where the kernels
    # skipped a splat both oracles kept - one pixel, four rows of dL/dmeans2d set aside.)
    margin = alpha_threshold_margin(c, o32)
    assert margin >= ALPHA_MARGIN, ("an alpha within fp32 rounding of 1/255", margin)
    return dict(mi, **mg, camera_worst=worst, alpha_margin=margin)


def population(c: Case, radii):
    """Per view: Gaussians visible (radius > 0 in `radii`), behind the camera (z <= 0), inside the 0.2 near cull (0 < z <= 0.2) and
    visible beyond the 1.3 tan-fov frustum clamp of the EWA Jacobian - from the records the kernels read, in fp32."""
    rows = []
    for v in range(c.cfg.num_views):
        f = c.vb[v].numpy()
        m = c.means[v // c.cfg.views_per_set].numpy() * f[40]
        cam = [f[k] * m[:, 0] + f[4 + k] * m[:, 1] + f[8 + k] * m[:, 2] + f[12 + k] for k in range(3)]
        z = cam[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            beyond = (np.abs(cam[0] / z) > np.float32(1.3) * f[35]) | (np.abs(cam[1] / z) > np.float32(1.3) * f[36])
        vis = np.asarray(radii[v]) > 0
        rows.append(dict(visible=int(vis.sum()), behind=int((z <= 0).sum()), near_culled=int(((z > 0) & (z <= np.float32(0.2))).sum()),
                         clamped=int((vis & beyond).sum())))
    return rows


def rig_properties(c: Case):
    """What the rig is for, on one case: raises AssertionError when a view's rotation has a small off-diagonal entry, when fx and fy of a
    view are within 5 %, or when two views of the call share a rotation, a tangent pair or a scale.  (scale: 1 / near under the
    scale-invariant rescale, where near is drawn from three values - hence part of the seed's selection; without the rescale every
    record's scale is 1 and the near planes are what must differ.)"""
    vb = c.vb.numpy()
    for v in range(vb.shape[0]):
        rot = vb[v, :16].reshape(4, 4)[:3, :3]
        off = np.abs(rot[~np.eye(3, dtype=bool)])
        assert off.min() >= 0.01, (v, rot)
        assert abs(vb[v, 35] / vb[v, 36] - 1.0) >= 0.05 and abs(vb[v, 36] / vb[v, 35] - 1.0) >= 0.05, (v, vb[v, 35:37])
    vps = c.cfg.views_per_set
    for a in range(vb.shape[0]):
        for b in range(a + 1, vb.shape[0]):
            assert np.abs(vb[a, :16] - vb[b, :16]).reshape(4, 4)[:3, :3].max() > 1e-3, (a, b)
            assert vb[a, 35] != vb[b, 35] and vb[a, 36] != vb[b, 36], (a, b)
            if a // vps == b // vps and vps <= len(NEARS):  # (the views of a set: read in one fused loop)
                assert vb[a, 43] != vb[b, 43], (a, b, "near")
                assert (vb[a, 40] != vb[b, 40]) or (vb[a, 40] == 1.0 and vb[b, 40] == 1.0), (a, b, "scale")
    if vps > len(NEARS):  # (more views in a set than there are near planes to draw: every one of them occurs)
        for s in range(c.cfg.num_sets):
            assert len(set(vb[s * vps:(s + 1) * vps, 43].tolist())) == len(NEARS), s


def alpha_pair(c: Case):
    """(fp32, fp64) references of a case with cfg.alpha: tests/test_alpha_gpu.py's two-run oracle, camera gradients included."""
    from tests.test_alpha_gpu import oracle_alpha

    g = torch.Generator().manual_seed(int(c.cfg.num_gaussians))
    ga = torch.rand((c.cfg.num_views, c.cfg.height, c.cfg.width), generator=g) - 0.3
    tup = (c.cfg, c.vb, c.means, c.cov, c.opac, c.colors, c.extra, c.frames)
    return ga, tuple(oracle_alpha(tup, c.gc, c.ge, ga, want_views=bool(c.want_views), dtype=dt) for dt in (np.float32, np.float64))


def alpha_guard(c: Case):
    """The seed guard for the accumulated-alpha case: the same conditions, the alpha image in the extra channel's place as well."""
    _, (o32, o64) = alpha_pair(c)
    m = seed_guard(c, o32, o64)
    res = dict(hip=dict(color=o32["color"], extra=o32["alpha"]), oracle=dict(color=o64["color"], extra=o64["alpha"]))
    ma = parity_checks.check_image(res, c.cfg)
    assert ma["outlier_pixels_1e-4"] == 0 and ma["extra_rel_l2_all"] < parity_checks.TOL, ma
    return m
