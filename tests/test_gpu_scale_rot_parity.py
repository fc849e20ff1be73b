"""The scale / rotation form on the MI355X against the CPU oracle and against itself: (S, N, 7) scale + quaternion records, per-set
`frames`, harmonics in those frames (GSR_FLAG_SH_IN_FRAME, both bases) - the form the fused adapter trains with - over random
shapes and several scenes (tests/fuzz_cases.py draw_sr_case); a batch of scenes against its single-scene calls bit for bit; the
fused adapter through the decoder at a batch of two scenes; the plan API's backward in this form."""
from collections import Counter

import numpy as np
import pytest
import torch

import pf3plat_amd
from pf3plat_amd import _lib, rasterizer, synthetic
from pf3plat_amd.adapter import GaussianAdapter, GaussianAdapterCfg
from pf3plat_amd.rasterizer import RasterConfig
from pf3plat_amd.sh_rotation import rotate_sh
from pf3plat_amd.types import Gaussians
from tests import gpu_util, parity_checks
from tests.fuzz_cases import draw_sr_case
from tests.test_gpu_sh_frame import _adapter_inputs
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DEPTH = 1 << 4  # GSR_FLAG_EXTRA_MODE(GSR_EXTRA_DEPTH)
SR_SEED, SR_CASES = 11, 72


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_randomised_scale_rotation_records_frames_and_scenes():
    """72 cases of `draw_sr_case` (seed 11): Gaussian counts 0 .. 20 000 at wave-size edges, images of 1 .. 160 px per side, 1-4 scenes x
    1-3 views, F = 1 / F = N / groups that straddle 64-lane units, SH degree 0-4 in either layout or precomputed colours, both SH-frame
    bases or none, extra channel (given or built in), windowed binning, BACKWARD_FOLLOWS (with the backward that takes the forward's
    rows), DETERMINISTIC, tiny pair capacities, camera gradients - each through every stage check, the image, the gradients (the records'
    and the frame harmonics') and the camera gradients.  A failure names its case: tests/fuzz_cases.py named_sr_case(11, k)."""
    hip = rasterizer.HipBackend()
    rng = np.random.default_rng(SR_SEED)
    seen, failed = Counter(), []
    for k in range(SR_CASES):
        desc, (cfg, vb, means, records, opac, colors, extra, gc, ge, cap, frames, sh_frame, want_views) = draw_sr_case(rng)
        n = cfg.num_gaussians
        print(f"named_sr_case({SR_SEED}, {k}): {desc}", flush=True)
        try:
            res = gpu_util.run_both(cfg, vb, means, records, opac, colors, extra, gc, ge, capacity=cap, want_views=want_views,
                                    frames=frames, sh_frame=sh_frame, rows_in_workspace=desc["follows"])
            if n:
                for v in range(cfg.num_views):
                    parity_checks.check_preprocess(res, cfg, v)
                    parity_checks.check_tile_lists(res, cfg, v, max_tiles=16)
                    parity_checks.check_image_state(res, cfg, v)
            parity_checks.check_image(res, cfg)
            if n:
                parity_checks.check_grads(res, cfg)
                if want_views:
                    parity_checks.check_camera_grads(res)
        except AssertionError as e:  # (every case runs: the report names all that fail)
            failed.append(f"named_sr_case({SR_SEED}, {k}): {desc}: {str(e)[:1500]}")
            print("FAILED", failed[-1], flush=True)
            continue
        if n:
            seen["colour_in_binning_%d" % hip.lib.gsr_colour_in_binning(hip._dims(cfg, 1 << 16))] += 1
            seen["sh_frame_" + str(sh_frame)] += 1
            seen["no_frames"] += frames is None
            seen["sets>=2_with_frames"] += cfg.num_sets >= 2 and frames is not None
            seen["F=N"] += n > 1 and frames is not None and frames.shape[1] == n
            seen["straddle"] += frames is not None and 1 < frames.shape[1] < n and (n // frames.shape[1]) % 64 != 0
            seen["windowed"] += desc["windowed"]
            seen["follows"] += desc["follows"]
            seen["det"] += desc["det"]
            seen["want_views_" + str(want_views)] += 1
        if n in (0, 1):
            seen[f"N={n}"] += 1
    print("coverage:", dict(seen))
    assert not failed, "\n".join(failed)
    for axis in ("sh_frame_e3nn", "sh_frame_rasterizer", "sh_frame_None", "no_frames", "sets>=2_with_frames", "F=N", "straddle", "N=0",
                 "N=1", "colour_in_binning_0", "colour_in_binning_1", "windowed", "follows", "det", "want_views_True", "want_views_depth"):
        assert seen[axis] >= 1, (axis, dict(seen))


def _batch_inputs(b_sets, n, hw, seed):
    scs = [synthetic.make_scene(seed + b, n, hw, num_views=3, d_sh=1, structure=("random", "pixel_aligned")[b & 1]) for b in range(b_sets)]
    g = torch.Generator().manual_seed(seed)
    means = torch.cat([sc.gaussians.means for sc in scs]).contiguous()
    opac = torch.cat([sc.gaussians.opacities for sc in scs]).contiguous()
    scales = (0.5 + 14.5 * torch.rand((b_sets, n, 3), generator=g)) * means.norm(dim=-1, keepdim=True) * (4.0 / (0.86 * hw[1]))
    records = torch.cat((scales, torch.randn((b_sets, n, 4), generator=g)), -1).contiguous()
    sh = 0.4 * torch.randn((b_sets, n, 3, 25), generator=g)  # PF3plat's planar harmonics
    q = torch.linalg.qr(torch.randn((b_sets, 2, 3, 3), dtype=torch.float64, generator=g))[0]
    frames = (q * torch.det(q)[..., None, None]).float().contiguous()  # two source views per scene, every scene its own
    vbs = [gpu_util.scene_viewbuf(sc) for sc in scs]
    return means, records, opac, sh, frames, vbs


@pytest.mark.parametrize("basis", ["e3nn", "rasterizer"])
def test_batch_of_scenes_with_frames_equals_single_scene_calls_bit_for_bit(basis):
    """The training call of the fused adapter (4 scenes x 3 views of 131 072 Gaussians as scale + quaternion records, F = 2 frames per
    scene, harmonics in those frames, colour + built-in depth, DETERMINISTIC): one call over the batch returns, scene by scene, the bits
    of the calls that render a scene alone - image, depth, radii, every Gaussian gradient and the camera gradients.  And the frames of
    scene s are what scene s reads: given scene 0's frames everywhere, the images of scenes 1-3 change."""
    b_sets, n, hw = 4, 131072, (256, 256)
    means, records, opac, sh, frames, vbs = _batch_inputs(b_sets, n, hw, 120)
    g = torch.Generator().manual_seed(121)
    gc = torch.rand((3 * b_sets, 3, *hw), generator=g)
    ge = torch.rand((3 * b_sets, *hw), generator=g)
    flags = DEPTH | _lib.FLAG_DETERMINISTIC | _lib.FLAG_SH_PLANAR
    cfg_b = RasterConfig(3 * b_sets, b_sets, 3, n, *hw, 4, 25, 4, True, flags, True)
    whole = gpu_util.run_hip(cfg_b, torch.cat(vbs), means, records, opac, sh, None, gc, ge, frames=frames, sh_frame=basis, want_views=True)
    assert not whole["status"]["overflow"]
    assert np.abs(whole["grads"]["views"]).max() > 0 and np.abs(whole["grads"]["colors"][..., 1:]).max() > 0
    cfg_1 = RasterConfig(3, 1, 3, n, *hw, 4, 25, 4, True, flags, True)
    for b in range(b_sets):
        s, v = slice(b, b + 1), slice(3 * b, 3 * b + 3)
        one = gpu_util.run_hip(cfg_1, vbs[b], means[s], records[s], opac[s], sh[s], None, gc[v], ge[v], frames=frames[s], sh_frame=basis,
                               want_views=True)
        for name in ("color", "extra"):
            assert np.array_equal(_bits(whole[name][v]), _bits(one[name])), (b, name)
        assert np.array_equal(whole["radii"][v], one["radii"]), b
        for name in ("means", "cov6", "opac", "colors"):
            assert np.array_equal(_bits(whole["grads"][name][s]), _bits(one["grads"][name])), (b, name)
        for name in ("means2d", "views"):
            assert np.array_equal(_bits(whole["grads"][name][v]), _bits(one["grads"][name])), (b, name)
    # teeth: a kernel that read scene 0's frames for every scene would render this
    wrong = gpu_util.run_hip(cfg_b, torch.cat(vbs), means, records, opac, sh, None, frames=frames[:1].expand(b_sets, -1, -1, -1).contiguous(),
                             sh_frame=basis)
    for b in range(1, b_sets):
        v = slice(3 * b, 3 * b + 3)
        assert rel_l2(wrong["color"][v], whole["color"][v]) > 1e-2, b
    assert np.array_equal(_bits(wrong["color"][0:3]), _bits(whole["color"][0:3]))


@pytest.mark.parametrize("basis", ["e3nn", "rasterizer"])
def test_fused_adapter_decoder_at_batch_two(basis):
    """`test_fused_adapter_end_to_end_at_pf3plat_size` at a batch of two scenes (2 source views x 128^2 pixel-aligned Gaussians each,
    3 target views per scene, colour + depth through DecoderSplattingCUDA): `Gaussians.for_decoder` and the decoder's reshaping of
    `frames` for b > 1 - the fused adapter against the default one (rotate_sh in torch)."""
    b, hs, ws = 2, 128, 128
    ext, intr, coords, depths, opac, raw0 = _adapter_inputs(seed=12, hs=hs, ws=ws, b=b)
    scs = [synthetic.make_scene(50 + k, 8, (256, 256), num_views=3) for k in range(b)]
    cams = [torch.cat([getattr(sc, a) for sc in scs]).to(DEV) for a in ("extrinsics", "intrinsics", "near", "far")]
    g = torch.Generator().manual_seed(8)
    w = torch.rand((b, 3, 3, 256, 256), generator=g).to(DEV)
    wd = (0.05 * torch.rand((b, 3, 256, 256), generator=g)).to(DEV)
    dec = pf3plat_amd.DecoderSplattingCUDA().to(DEV)
    cfg = GaussianAdapterCfg(0.5, 15.0, 4)
    res = []
    for fused in (True, False):
        ad = GaussianAdapter(cfg, fuse_sh_rotation=True, sh_basis=basis) if fused else \
            GaussianAdapter(cfg, rotate_sh=lambda s, r: rotate_sh(s, r, basis=basis))
        raw = raw0.clone().requires_grad_(True)
        out = ad.forward(ext[:, :, None], intr[:, :, None], coords, depths, opac, raw, (hs, ws))
        gs = out.for_decoder()
        mv = lambda x: None if x is None else x.to(DEV)
        gs = Gaussians(mv(gs.means), None, mv(gs.harmonics), mv(gs.opacities), mv(gs.scales), mv(gs.rotations), mv(gs.frames), gs.sh_frame)
        assert gs.sh_frame == (basis if fused else None) and gs.means.shape == (b, 2 * hs * ws, 3)
        if fused:
            assert gs.frames.shape == (b, 2, 3, 3) and not torch.equal(gs.frames[0], gs.frames[1])
        o = dec.forward(gs, *cams, (256, 256), depth_mode="depth")
        ((o.color * w).sum() + (o.depth * wd).sum()).backward()
        res.append((o.color.detach().cpu().numpy(), o.depth.detach().cpu().numpy(), raw.grad.cpu().numpy()))
    for k in range(b):
        assert np.abs(res[1][0][k]).max() > 0.1 and np.abs(res[1][2][k, ..., 7:]).max() > 0, k
        assert rel_l2(res[0][0][k], res[1][0][k]) <= 1e-5 and rel_l2(res[0][1][k], res[1][1][k]) <= 1e-5, k
        assert rel_l2(res[0][2][k], res[1][2][k]) <= 1e-4, k


@pytest.mark.parametrize("follows", [False, True])
def test_plan_api_backward_in_the_scale_rotation_form(follows):
    """The plan API (make_plan(backward=True), run_forward, run_backward) in the scale / rotation form with frames and harmonics in
    them (e3nn basis), 2 scenes x 2 views, 750-Gaussian groups that straddle units, DETERMINISTIC: three forward + backward steps on one
    plan - the third with camera gradients (gsr_backward_ex) - each bit-equal to HipBackend.forward / backward on the same inputs."""
    hip = rasterizer.HipBackend()
    sets, vps, n, hw = 2, 2, 3000, (64, 72)
    scs = [synthetic.make_scene(140 + s, n, hw, num_views=vps, d_sh=1) for s in range(sets)]
    g = torch.Generator().manual_seed(140)
    means = torch.cat([sc.gaussians.means for sc in scs]).contiguous()
    opac = torch.cat([sc.gaussians.opacities for sc in scs]).contiguous()
    scales = (0.5 + 14.5 * torch.rand((sets, n, 3), generator=g)) * means.norm(dim=-1, keepdim=True) * (4.0 / (0.86 * hw[1]))
    records = torch.cat((scales, torch.randn((sets, n, 4), generator=g)), -1)
    sh = 0.4 * torch.randn((sets, n, 3, 16), generator=g)
    q = torch.linalg.qr(torch.randn((sets, 4, 3, 3), dtype=torch.float64, generator=g))[0]
    frames = (q * torch.det(q)[..., None, None]).float()
    vb = torch.cat([gpu_util.scene_viewbuf(sc) for sc in scs]).to(DEV)
    means, records, opac, sh, frames = (x.to(DEV).contiguous() for x in (means, records, opac, sh, frames))
    flags = DEPTH | _lib.FLAG_DETERMINISTIC | _lib.FLAG_SH_PLANAR | gpu_util.SH_FRAME_BITS["e3nn"] | \
        (_lib.FLAG_BACKWARD_FOLLOWS if follows else 0)
    cfg = RasterConfig(sets * vps, sets, vps, n, *hw, 3, 16, 4, True, flags, True)
    hip.forward(cfg, vb, means, records, opac, sh, None, frames=frames)
    plan = hip.make_plan(cfg, DEV, 2 * int(hip.last_status["num_pairs"]) + 1024, backward=True)
    names = ("d_means", "d_cov6", "d_opac", "d_colors", "d_means2d")
    for step in range(3):
        gc = torch.rand((sets * vps, 3, *hw), generator=g).to(DEV)
        ge = torch.rand((sets * vps, *hw), generator=g).to(DEV)
        want_views = step == 2
        hip.run_forward(plan, vb, means, records, opac, sh, None, frames=frames)
        d_views = torch.empty((sets * vps, rasterizer.VIEW_FLOATS), device=DEV) if want_views else None
        hip.run_backward(plan, vb, means, records, opac, sh, None, gc, ge, frames=frames, d_views=d_views)
        torch.cuda.synchronize()
        assert not hip.read_status(plan)["overflow"]
        got = {k: plan[k].cpu().numpy() for k in ("color", "extra_img", "radii") + names}
        c, e, r, saved = hip.forward(cfg, vb, means, records, opac, sh, None, frames=frames)
        want = hip.backward(cfg, saved, vb, means, records, opac, sh, None, gc, ge, True, rows_in_workspace=follows, frames=frames,
                            want_views=want_views)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(got["color"]), _bits(c.cpu().numpy())), step
        assert np.array_equal(_bits(got["extra_img"]), _bits(e.cpu().numpy())), step
        assert np.array_equal(got["radii"], r.cpu().numpy()), step
        for k, name in enumerate(names[:4]):
            assert np.array_equal(_bits(got[name]), _bits(want[k].cpu().numpy())), (step, name)
        assert np.array_equal(_bits(got["d_means2d"]), _bits(want[5].cpu().numpy())), step
        assert np.abs(got["d_colors"][..., 1:]).max() > 0, step
        if want_views:
            assert np.abs(want[6].cpu().numpy()).max() > 0
            assert np.array_equal(_bits(d_views.cpu().numpy()), _bits(want[6].cpu().numpy())), step
