"""Accumulated alpha A = sum_j alpha_j T_j = 1 - T_final on the MI355X (GsrForwardOptions.out_alpha / GsrBackwardOptions.dL_dalpha_img) against the CPU oracle.

The oracle is untouched.  A is what its fp32 instantiation blends for a caller-supplied extra channel of ones; the backward being
linear in the incoming image gradients over a fixed forward, the reference for (g_color, g_extra, g_A) is the sum of two oracle backwards
on the same scene: the call's own (g_color, g_extra) and one with extra = ones, g_color = 0, g_extra = g_A (dL_dextra from the first
only).  Tolerances are tests/parity_checks.py's: rel-L2 < 1e-4 over all pixels / gradient rows, its set-aside rule for flipped threshold
pixels with its cap.  Max-abs error of A: HIP's distance to the fp64 oracle must be within twice the fp32 oracle's own distance to it on
the same case (1 - T and sum alpha T round differently); the measured values of both are in docs/PARITY.md, section 7.

Seeds (every case below): chosen so that the fp32 oracle against the fp64 oracle stays within parity_checks' caps on its own
(`oracle32_vs_oracle64`, run on the CPU when the cases were written): 31 (case 1), 32 (case 2), 33 (saturation), 34 / 35 (long lists),
36 (compact), 37 (camera gradients), 38 (decoder)."""
import dataclasses

import numpy as np
import pytest
import torch

from pf3plat_amd import _lib, rasterizer, splatting, synthetic
from pf3plat_amd.decoder import DecoderSplattingCUDA
from pf3plat_amd.rasterizer import RasterConfig
from tests import gpu_util, parity_checks

pytestmark = pytest.mark.gpu
DEPTH = 1 << 4  # GSR_FLAG_EXTRA_MODE(GSR_EXTRA_DEPTH)
GRADS = ("means", "cov6", "opac", "colors", "extra", "means2d", "views")


# ---- cases: (cfg with alpha=True, viewbuf, means, cov, opac, colors, extra, frames), all CPU tensors ---------------------------------
def _rand_grads(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    v, hw = cfg.num_views, (cfg.height, cfg.width)
    return (torch.rand((v, 3, *hw), generator=g), torch.rand((v, *hw), generator=g) if cfg.has_extra else None,
            torch.rand((v, *hw), generator=g) - 0.3)


def case_colour_only(flags=0):
    """1 view, 64 x 64, N = 256, SH degree 4, background (0.3, 0.5, 0.7), no extra channel."""
    sc = synthetic.make_scene(31, 256, (64, 64))
    sc.background = torch.tensor([0.3, 0.5, 0.7])
    means, cov6, opac, colors = gpu_util.scene_tensors(sc)
    return RasterConfig(1, 1, 1, 256, 64, 64, 4, 25, 4, False, flags, False, True), gpu_util.scene_viewbuf(sc), means, cov6, opac, colors, None, None


def case_two_sets(flags=0):
    """2 sets x 3 views, N = 1000, 72 x 40, scale + quaternion records in F = 2 frames per set, planar harmonics, built-in depth."""
    n, hw = 1000, (72, 40)
    scs = [synthetic.make_scene(32 + 100 * b, n, hw, num_views=3, d_sh=1) for b in range(2)]
    g = torch.Generator().manual_seed(32)
    means = torch.cat([sc.gaussians.means for sc in scs]).contiguous()
    opac = torch.cat([sc.gaussians.opacities for sc in scs]).contiguous()
    scales = (0.5 + 14.5 * torch.rand((2, n, 3), generator=g)) * means.norm(dim=-1, keepdim=True) * (4.0 / (0.86 * hw[1]))
    records = torch.cat((scales, torch.randn((2, n, 4), generator=g)), -1).contiguous()
    sh = 0.4 * torch.randn((2, n, 3, 25), generator=g)
    q = torch.linalg.qr(torch.randn((2, 2, 3, 3), dtype=torch.float64, generator=g))[0]
    frames = (q * torch.det(q)[..., None, None]).float().contiguous()
    vb = torch.cat([gpu_util.scene_viewbuf(sc) for sc in scs])
    cfg = RasterConfig(6, 2, 3, n, *hw, 4, 25, 4, True, DEPTH | _lib.FLAG_SH_PLANAR | flags, True, True)
    return cfg, vb, means, records, opac, sh, None, frames


def case_saturated():
    """64 x 64, 256 Gaussians: large near-opaque splats on the left of the image (nearly half the pixels they reach stop early), nothing on its
    right (every Gaussian that would project there is moved behind the camera, with 16 more: their rows must stay exactly 0)."""
    sc = synthetic.make_scene(33, 256, (64, 64), d_sh=1)
    means, cov6, opac, colors = gpu_util.scene_tensors(sc, use_sh=False)
    means, cov6, opac = means.clone(), cov6 * 16.0, torch.full_like(opac, 0.99)
    px = 0.86 * means[0, :, 0] / means[0, :, 2] + 0.5  # normalised image x of every centre (camera 0 is the identity)
    behind = (px > 0.3) | (torch.arange(256) >= 240)
    means[0, behind] *= -1.0
    cfg = RasterConfig(1, 1, 1, 256, 64, 64, 0, 0, 4, False, 0, False, True)
    return (cfg, gpu_util.scene_viewbuf(sc), means, cov6.contiguous(), opac, colors, None, None), behind


def case_stacked(n, seed):
    """32 x 32, n small faint Gaussians stacked on the pixels around (12, 12): one tile list of about n entries."""
    sc = synthetic.make_scene(seed, n, (32, 32), d_sh=1)
    g = torch.Generator().manual_seed(seed)
    z = 2.0 + 6.0 * torch.rand(n, generator=g)
    uv = (torch.tensor([12.5, 12.5]) + 1.5 * torch.randn((n, 2), generator=g)) / 32.0
    means = (torch.stack(((uv[:, 0] - 0.5) / 0.86, (uv[:, 1] - 0.5) / 0.86, torch.ones(n)), -1) * z[:, None])[None].contiguous()
    s2 = (1.2 * z / (0.86 * 32.0)) ** 2
    cov6 = torch.zeros((1, n, 6))
    cov6[0, :, 0] = cov6[0, :, 3] = cov6[0, :, 5] = s2
    opac = (0.006 + 0.01 * torch.rand((1, n), generator=g))
    colors = torch.rand((1, n, 3), generator=g)
    cfg = RasterConfig(1, 1, 1, n, 32, 32, 0, 0, 4, False, 0, False, True)
    return cfg, gpu_util.scene_viewbuf(sc), means, cov6, opac, colors, None, None


def case_many_tiles():
    """One 320 x 264 image: 1360 tiles, more than the 1280 from which the tile launch takes its compact instance."""
    sc = synthetic.make_scene(36, 2000, (264, 320), d_sh=1)
    means, cov6, opac, colors = gpu_util.scene_tensors(sc, use_sh=False)
    return RasterConfig(1, 1, 1, 2000, 264, 320, 0, 0, 4, False, 0, False, True), gpu_util.scene_viewbuf(sc), means, cov6, opac, colors, None, None


def case_cameras():
    """2 views, 64 x 64, N = 500, degree-4 harmonics, built-in depth: the call the camera gradients are asked of."""
    sc = synthetic.make_scene(37, 500, (64, 64), num_views=2)
    means, cov6, opac, colors = gpu_util.scene_tensors(sc)
    return RasterConfig(2, 1, 2, 500, 64, 64, 4, 25, 4, True, DEPTH, False, True), gpu_util.scene_viewbuf(sc), means, cov6, opac, colors, None, None


# ---- both sides -----------------------------------------------------------------------------------------------------------------------
def oracle_alpha(case, gc=None, ge=None, ga=None, want_views=False, dtype=np.float32):
    """The reference: -> dict(color, extra, alpha, handles[, grads]) from the two oracle runs described at the top."""
    cfg, vb, means, cov, opac, colors, extra, frames = case
    cfg = dataclasses.replace(cfg, alpha=False)
    ones_cfg = dataclasses.replace(cfg, has_extra=True, flags=cfg.flags & ~0x70)
    ones = torch.ones((cfg.num_views, cfg.num_gaussians))
    zero = None if gc is None else torch.zeros_like(gc)
    own = gpu_util.run_oracle(cfg, vb, means, cov, opac, colors, extra, gc, ge, dtype, True, want_views, frames)
    acc = gpu_util.run_oracle(ones_cfg, vb, means, cov, opac, colors, ones, zero, ga, dtype, True, want_views, frames)
    out = dict(color=own["color"], extra=own["extra"], alpha=acc["extra"], radii=own["radii"], handles=own["handles"])
    if gc is not None:
        out["grads"] = {k: (own["grads"].get(k) if k == "extra" or own["grads"].get(k) is None else own["grads"][k] + acc["grads"][k]) for k in GRADS}
    return out


def hip_alpha(case, gc=None, ge=None, ga=None, want_views=False, follows=False, capacity=None):
    cfg, vb, means, cov, opac, colors, extra, frames = case
    dev = torch.device("cuda:0")
    hip = rasterizer.HipBackend()
    to = lambda t: None if t is None else t.to(dev).contiguous()
    args = tuple(to(a) for a in (means, cov, opac, colors, extra))
    color, extra_img, radii, saved, alpha = hip.forward(cfg, to(vb), *args, capacity=capacity, frames=to(frames))
    torch.cuda.synchronize()
    out = dict(color=color.cpu().numpy(), extra=None if extra_img is None else extra_img.cpu().numpy(), alpha=alpha.cpu().numpy(),
               radii=radii.cpu().numpy(), capacity=int(saved[0].pair_capacity))
    # (the capacity the call ran with decides the tile kernel - gsr_hip.hip forward_impl: entries per tile = capacity / (2 views tiles),
    # windowed chain: capacity / (views tiles) - so a test that names an instance checks that its capacity was not outgrown and retried)
    assert capacity is None or out["capacity"] == capacity, (capacity, out["capacity"])
    if cfg.num_gaussians:
        out.update(ws=gpu_util.decode_workspaces(hip, cfg, saved), status=hip.last_status)
        assert not out["status"]["overflow"]
    if gc is not None:
        g = hip.backward(cfg, saved, to(vb), *args, to(gc), to(ge), True, rows_in_workspace=follows, frames=to(frames), want_views=want_views,
                         g_alpha_img=to(ga))
        torch.cuda.synchronize()
        out["grads"] = {k: (None if t is None else t.cpu().numpy()) for k, t in zip(GRADS, g)}
    return out


def check_alpha_image(h, o, o64=None):
    """A against the oracle's blend of ones: parity_checks' image rule (rel-L2 < 1e-4, its cap on outlier pixels), every value in
    [0, 1), and - given the fp64 oracle's A - the max-abs bound: HIP within twice the fp32 oracle's own distance to fp64."""
    res = dict(hip=dict(color=h["color"], extra=h["alpha"]), oracle=dict(color=o["color"], extra=o["alpha"]))
    cfg = None
    m = parity_checks.check_image(res, cfg)
    assert np.isfinite(h["alpha"]).all() and h["alpha"].min() >= 0.0 and h["alpha"].max() < 1.0
    if o64 is not None:
        d32 = float(np.abs(o["alpha"].astype(np.float64) - o64["alpha"]).max())
        dh = float(np.abs(h["alpha"].astype(np.float64) - o64["alpha"]).max())
        print(f"alpha max-abs vs fp64 oracle: fp32 oracle {d32:.3e}, HIP {dh:.3e}")
        m["alpha_max_abs_oracle32"], m["alpha_max_abs_hip"] = d32, dh
        assert dh <= 2.0 * d32, m
    return m


def check_all(case, h, o, o64=None):
    cfg = case[0]
    res = dict(hip=h, oracle=o)
    m = parity_checks.check_image(res, cfg)
    m.update(check_alpha_image(h, o, o64))
    if "grads" in h:
        hg = {k: v for k, v in h["grads"].items() if k != "views"}
        og = {k: v for k, v in o["grads"].items() if k != "views"}
        m.update(parity_checks.check_grads(dict(hip=dict(h, grads=hg), oracle=dict(o, grads=og)), cfg))
    print({k: v for k, v in m.items() if k.endswith("rel_l2_all") or k.endswith("set_aside") or k.startswith("alpha_")})
    return m


def oracle32_vs_oracle64(case, seed=0):
    """How the seeds were chosen (CPU): the fp32 oracle in HIP's place against the fp64 oracle, through the same checks."""
    gc, ge, ga = _rand_grads(case[0], seed)
    o32, o64 = oracle_alpha(case, gc, ge, ga), oracle_alpha(case, gc, ge, ga, dtype=np.float64)
    h = dict(o32, ws=dict(final_T=np.stack([hd[0].image_state()["final_T"] for hd in o32["handles"][:case[0].num_views]])))
    return check_all(case, h, o64)


# ---- 1: colour only -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def colour_case():
    case = case_colour_only()
    gc, _, ga = _rand_grads(case[0], 1)
    return case, gc, ga, oracle_alpha(case, gc, None, ga), oracle_alpha(case, torch.zeros_like(gc), None, ga), oracle_alpha(case, dtype=np.float64)


# capacities: the default (k_tile_fwd_prefix), 512 entries per tile (k_tile_fwd<gather, 2048>), 8192 per tile (k_tile_fwd<gather, 4096>)
@pytest.mark.parametrize("capacity", [None, 2 * 64 * 512, 2 * 64 * 8192])
def test_colour_only_alpha_and_gradients(colour_case, capacity):
    case, gc, ga, o_both, o_alone, o64 = colour_case
    h = hip_alpha(case, gc, None, ga, capacity=capacity)
    check_all(case, h, o_both, o64)
    assert float(h["alpha"].max()) > 0.5 and float(h["alpha"].min()) < 0.5
    # colour = blended + (1 - A) bg: with the background in, the image is not the one without it
    if capacity is None:
        h0 = hip_alpha(case, torch.zeros_like(gc), None, ga)  # a loss on A alone: zeros for dL_dcolor
        m = check_all(case, h0, o_alone)
        assert m["opac_norm"] > 0 and m["means_norm"] > 0
        assert np.array_equal(h0["alpha"], h["alpha"])


def test_windowed_binning_on_a_small_image(colour_case):
    _, gc, ga, o_both, _, o64 = colour_case
    for capacity in (None, 2 * 64 * 256):  # k_tile_fwd<no gather, 4096 | 2048>
        case = case_colour_only(_lib.FLAG_WINDOWED_BINNING)
        check_all(case, hip_alpha(case, gc, None, ga, capacity=capacity), o_both, o64)


# ---- 2: two sets x three views, records with frames, built-in depth ---------------------------------------------------------------
@pytest.fixture(scope="module")
def two_sets():
    case = case_two_sets()
    gc, ge, ga = _rand_grads(case[0], 2)
    return gc, ge, ga, oracle_alpha(case, gc, ge, ga), oracle_alpha(case, dtype=np.float64)


# 6 views x 60 tiles at the default capacity: 2184 entries per tile, k_tile_fwd<gather, 4096, extra>; with windowed binning
# 4369 per tile, k_tile_fwd<no gather, 4096, extra>
@pytest.mark.parametrize("follows,windowed", [(False, False), (True, False), (False, True)])
def test_two_sets_depth_and_alpha_in_the_scale_rotation_form(two_sets, follows, windowed):
    gc, ge, ga, o, o64 = two_sets
    case = case_two_sets((_lib.FLAG_BACKWARD_FOLLOWS if follows else 0) | (_lib.FLAG_WINDOWED_BINNING if windowed else 0))
    h = hip_alpha(case, gc, ge, ga, follows=follows)
    check_all(case, h, o, o64)
    # expected depth = depth / A where something was rendered: inside the depth range of the scene
    seen = h["alpha"] > 0.5
    assert seen.any() and (h["extra"][seen] / h["alpha"][seen] > 0.5).all() and (h["extra"][seen] / h["alpha"][seen] < 25.0).all()


def test_deterministic_backward_with_alpha_repeats_bit_for_bit(two_sets):
    gc, ge, ga, _, _ = two_sets
    case = case_two_sets(_lib.FLAG_DETERMINISTIC)
    a, b = hip_alpha(case, gc, ge, ga), hip_alpha(case, gc, ge, ga)
    for k in GRADS[:6]:
        if a["grads"][k] is not None:
            assert np.array_equal(a["grads"][k].view(np.uint32), b["grads"][k].view(np.uint32)), k
    # and g_A is in them: without it the gradients are others
    c = hip_alpha(case, gc, ge, torch.zeros_like(ga))
    assert not np.array_equal(a["grads"]["opac"], c["grads"]["opac"])


# ---- 3: saturation, empty region, empty call ----------------------------------------------------------------------------------------
def test_saturated_pixels_empty_region_and_untouched_rows():
    case, behind = case_saturated()
    gc, _, ga = _rand_grads(case[0], 3)
    o, o64 = oracle_alpha(case, gc, None, ga), oracle_alpha(case, dtype=np.float64)
    h = hip_alpha(case, gc, None, ga)
    check_all(case, h, o, o64)
    n_contrib = np.stack([hd[0].image_state()["n_contrib"] for hd in o["handles"]])
    final_T = np.stack([hd[0].image_state()["final_T"] for hd in o["handles"]])
    empty = n_contrib == 0
    assert empty.mean() > 0.15 and (final_T[~empty] < 1e-2).mean() > 0.4  # a region nothing reaches; many of the other pixels stop early
    assert not h["alpha"][empty].any() and not o["alpha"][empty].any()  # exactly 0
    assert h["alpha"][~empty].min() > 0
    # a pixel that stopped early keeps the T in front of the rejected splat: A stays below 1, and colour = blended + (1 - A) bg holds
    assert h["alpha"].max() < 1.0 and (h["alpha"] > 0.999).any()
    assert np.array_equal(h["alpha"], 1.0 - h["ws"]["final_T"])
    untouched = behind.numpy()
    assert untouched.sum() >= 16 and not (h["radii"][0][untouched] > 0).any()
    for k in ("means", "cov6", "opac", "colors"):
        assert not h["grads"][k][0][untouched].any(), k
        assert h["grads"][k][0][~untouched].any(), k


def test_empty_call_gives_an_all_zero_alpha_image():
    case, _ = case_saturated()
    cfg, vb, means, cov6, opac, colors, _, _ = case
    cfg0 = dataclasses.replace(cfg, num_gaussians=0)
    h = hip_alpha((cfg0, vb, means[:, :0], cov6[:, :0], opac[:, :0], colors[:, :0], None, None))
    assert h["alpha"].shape == (1, 64, 64) and not h["alpha"].any() and not h["color"].any()


# ---- 4: long lists, many tiles --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(700, 34), (2600, 35)])
def test_long_tile_lists(n, seed):
    case = case_stacked(n, seed)
    gc, _, ga = _rand_grads(case[0], 4)
    h = hip_alpha(case, gc, None, ga)
    assert h["status"]["max_list"] > (512 if n < 2048 else 2048), h["status"]
    check_all(case, h, oracle_alpha(case, gc, None, ga), oracle_alpha(case, dtype=np.float64))


def test_more_than_1280_tiles_takes_the_compact_instance():
    case = case_many_tiles()
    gc, _, ga = _rand_grads(case[0], 5)
    h = hip_alpha(case, gc, None, ga)
    assert h["ws"]["T"] > 1280
    check_all(case, h, oracle_alpha(case, gc, None, ga), oracle_alpha(case, dtype=np.float64))


# ---- the 2048-key instances with the extra channel: 2 views x 64 tiles, about 6 000 pairs ------------------------------------------
# 512 entries per tile: k_tile_fwd<gather, 2048, extra>; windowed binning at 600 per tile: k_tile_fwd<no gather, 2048, extra>
@pytest.mark.parametrize("windowed,capacity", [(False, 2 * 128 * 512), (True, 128 * 600)])
def test_short_list_instances_with_depth_and_alpha(windowed, capacity):
    case = case_cameras()
    gc, ge, ga = _rand_grads(case[0], 7)
    o, o64 = oracle_alpha(case, gc, ge, ga), oracle_alpha(case, dtype=np.float64)
    if windowed:
        case = (dataclasses.replace(case[0], flags=case[0].flags | _lib.FLAG_WINDOWED_BINNING),) + case[1:]
    check_all(case, hip_alpha(case, gc, ge, ga, capacity=capacity), o, o64)


# ---- 6: camera gradients --------------------------------------------------------------------------------------------------------------
def test_camera_gradients_carry_the_alpha_term():
    case = case_cameras()
    gc, ge, ga = _rand_grads(case[0], 6)
    o = oracle_alpha(case, gc, ge, ga, want_views=True)
    h = hip_alpha(case, gc, ge, ga, want_views=True)
    check_all(case, h, o)
    parity_checks.check_camera_grads(dict(hip=h, oracle=o))
    h0 = hip_alpha(case, gc, ge, torch.zeros_like(ga), want_views=True)
    assert not np.array_equal(h0["grads"]["views"], h["grads"]["views"])  # (the term is there)


# ---- 7: through the decoder -----------------------------------------------------------------------------------------------------------
def test_decoder_alpha_matches_the_c_abi_and_off_is_the_plain_path():
    dev = torch.device("cuda:0")
    n, hw, wc, wd, wa = 600, (48, 40), 0.7, 0.2, -0.4
    sc = synthetic.make_scene(38, n, hw, num_views=2).to(dev)
    dec = DecoderSplattingCUDA(on_overflow=None)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)  # (the backward's accumulation in fixed point: gradients comparable bit for bit)
    try:
        def run(alpha):
            g = sc.gaussians.clone()
            leaves = [t.requires_grad_(True) for t in (g.means, g.covariances, g.harmonics, g.opacities)]
            out = dec.forward(g, sc.extrinsics, sc.intrinsics, sc.near, sc.far, hw, depth_mode="depth", alpha=alpha)
            loss = (wc * out.color).sum() + (wd * out.depth).sum() + ((wa * out.alpha).sum() if alpha else 0.0)
            loss.backward()
            return out, [t.grad.clone() for t in leaves]

        on, g_on = run(True)
        off, g_off = run(False)
        assert off.alpha is None and on.alpha.shape == (1, 2, *hw) and on.alpha.requires_grad
        assert torch.equal(on.color, off.color) and torch.equal(on.depth, off.depth)
        # the same calls through the C ABI
        vb = splatting._viewbuf(sc.extrinsics[0], sc.intrinsics[0], sc.near[0], sc.far[0], dec.background_color.to(dev), True)
        g = sc.gaussians
        flags = DEPTH | _lib.FLAG_SH_PLANAR | _lib.FLAG_COV_3X3 | _lib.FLAG_DETERMINISTIC | _lib.FLAG_BACKWARD_FOLLOWS
        hip = rasterizer.HipBackend()
        args = (vb, g.means.contiguous(), g.covariances.contiguous(), g.opacities.contiguous(), g.harmonics.contiguous(), None)
        gc, ge, ga = (torch.full(s, w, device=dev) for s, w in (((2, 3, *hw), wc), ((2, *hw), wd), ((2, *hw), wa)))
        for alpha, out, grads in ((True, on, g_on), (False, off, g_off)):
            cfg = RasterConfig(2, 1, 2, n, *hw, 4, 25, 4, True, flags, False, alpha)
            color, depth, _, saved, *acc = hip.forward(cfg, *args)
            d = hip.backward(cfg, saved, *args, gc, ge, False, rows_in_workspace=True, g_alpha_img=ga if alpha else None)
            torch.cuda.synchronize()
            assert torch.equal(out.color[0], color) and torch.equal(out.depth[0], depth)
            if alpha:
                assert torch.equal(out.alpha[0], acc[0])
            else:
                assert not acc
            for name, a, b in zip(("means", "cov", "harmonics", "opac"), grads, (d[0], d[1], d[3], d[2])):
                assert torch.equal(a, b), (alpha, name)
        assert not torch.equal(g_on[3], g_off[3])
    finally:
        torch.use_deterministic_algorithms(was)
