"""The random cases of the parity fuzz (tools/fuzz_parity.py) as a replayable sequence: case k of seed s is a pure function of
(s, k) - the draws of a case do not depend on any result - so the worst cases a survey finds can be named and re-run
(`named_case(seed, index)`; the regression cases of tests/test_gpu_parity.py and the rows of tools/parity_vs_fp64.py).
Test infrastructure only."""
from __future__ import annotations

import numpy as np
import torch

from pf3plat_amd import _lib, synthetic
from pf3plat_amd.rasterizer import RasterConfig
from tests import gpu_util


def draw_case(rng, build: bool = True, structure: str = "random"):
    """One random case: -> (desc, inputs) with inputs = (cfg, viewbuf, means, cov6, opac, colors, extra, g_color, g_extra, capacity),
    all CPU tensors.  build=False makes exactly the same draws (the generator ends in the same state) without building anything:
    -> (desc, None).  structure="pixel_aligned" (round 6): the same draws, but the scene is the encoder-structured one
    (synthetic.make_scene(structure="pixel_aligned")) with the largest square source grid of at most n / 2 pixels - raster-ordered
    Gaussians, long (row, tile) runs; no extra random draw, so case (seed, k) names the same shape in both modes."""
    n = int(rng.choice([0, 1, 7, 63, 64, 65, 500, 1023, 1024, 1025, 3000, 9000, 20000]))
    h, w = int(rng.integers(1, 161)), int(rng.integers(1, 161))
    if rng.random() < 0.15:
        h, w = int(rng.choice([8, 16, 64, 128])), int(rng.choice([8, 16, 64, 128]))
    sets = int(rng.choice([1, 1, 2]))
    vps = int(rng.choice([1, 1, 2, 3]))
    views = sets * vps
    d_sh = int(rng.choice([1, 4, 9, 16, 25]))
    use_sh = bool(rng.random() < 0.8)
    with_extra = bool(rng.random() < 0.5)
    windowed = bool(rng.random() < 0.2)
    seed = int(rng.integers(0, 1 << 30))
    nears = [float(rng.choice([1.0, 0.5, 2.0])) for _ in range(sets)]
    scale_inv = [bool(rng.random() < 0.7) for _ in range(sets)]
    extra_np = rng.uniform(0.5, 2.0, (views, n)).astype(np.float32) if with_extra else None
    side = int(np.sqrt(n // 2)) if structure == "pixel_aligned" else 0
    if side >= 2:  # (smaller cases stay independently drawn)
        n = 2 * side * side
        extra_np = extra_np[:, :n].copy() if extra_np is not None else None
    deg = int(round(d_sh ** 0.5)) - 1
    flags = _lib.FLAG_WINDOWED_BINNING if windowed else 0
    # native layouts and built-in extra modes (depth / disparity / relative disparity / log from the camera-space depth)
    planar = bool(use_sh and rng.random() < 0.4)
    cov33 = bool(rng.random() < 0.4)
    emode = int(rng.integers(1, 5)) if (with_extra and rng.random() < 0.4) else 0
    follows = bool(rng.random() < 0.5)  # the forward saves d rgb / d direction and the backward uses it instead of the harmonics
    det = bool(rng.random() < 0.2)  # 64-bit fixed-point accumulators in the backward blend
    gc_np = rng.uniform(0, 1, (views, 3, h, w)).astype(np.float32)
    ge_np = rng.uniform(0, 1, (views, h, w)).astype(np.float32) if with_extra else None
    cap = None if rng.random() < 0.7 else int(rng.integers(1, 5000))
    desc = dict(n=n, hw=(h, w), sets=sets, vps=vps, d_sh=d_sh, use_sh=use_sh, extra=with_extra, windowed=windowed, seed=seed, cap=cap,
                planar=planar, cov33=cov33, emode=emode, follows=follows, det=det)
    if not build:
        return desc, None
    kw = dict(structure="pixel_aligned", source_shape=(side, side)) if side >= 2 else {}
    scs = [synthetic.make_scene(seed + s, n, (h, w), num_views=vps, d_sh=d_sh, near=nears[s], **kw) for s in range(sets)]
    parts = [gpu_util.scene_tensors(sc, use_sh) for sc in scs]
    means, cov6, opac, colors = (torch.cat([p[k] for p in parts], 0) for k in range(4))
    vb = torch.cat([gpu_util.scene_viewbuf(sc, scale_inv[s]) for s, sc in enumerate(scs)], 0)
    extra = torch.tensor(extra_np) if with_extra else None
    if planar:
        flags |= _lib.FLAG_SH_PLANAR
        colors = colors.permute(0, 1, 3, 2).contiguous()
    if cov33:
        flags |= _lib.FLAG_COV_3X3
        c = cov6
        cov6 = torch.stack((c[..., 0], c[..., 1], c[..., 2], c[..., 1], c[..., 3], c[..., 4], c[..., 2], c[..., 4], c[..., 5]), -1).reshape(*c.shape[:-1], 3, 3).contiguous()
    if emode:
        flags |= emode << 4
        extra = None
    if follows:
        flags |= _lib.FLAG_BACKWARD_FOLLOWS
    if det:
        flags |= _lib.FLAG_DETERMINISTIC
    cfg = RasterConfig(views, sets, vps, n, h, w, deg if use_sh else 0, d_sh if use_sh else 0, 4, with_extra, flags)
    gc = torch.tensor(gc_np)
    ge = torch.tensor(ge_np) if with_extra else None
    return desc, (cfg, vb, means, cov6, opac, colors, extra, gc, ge, cap)


def named_case(seed: int, index: int):
    """Case `index` of the sequence `np.random.default_rng(seed)` generates (the numbering of the survey's reports)."""
    rng = np.random.default_rng(seed)
    for _ in range(index):
        draw_case(rng, build=False)
    return draw_case(rng, build=True)


# The worst cases of the surveys so far, by (seed, index): every one is one or two pixels whose threshold decision (alpha < 1/255,
# T < 1e-4) falls the other way at fp32 rounding.  profiles/r04_m_fuzz_histogram_final_tree.md (seeds 7, 8), r04_fuzz_histogram.md (seed 4).
WORST_CASES = ((8, 275), (8, 886), (7, 151), (7, 332), (7, 885), (7, 844), (8, 75), (7, 695), (4, 363))


# ---- the scale / rotation form (gsr_forward_ex / gsr_backward_ex with scale_rot): a sequence of its
# own, so that draw_case's sequence - and every (seed, index) named above and in profiles/ - stays where it is
SR_SH_FRAMES = (None, "rasterizer", "e3nn")


def _sr_frame_count(n: int, kind: str, pick: float) -> int:
    """F for `kind`: "one" (F = 1), "each" (F = N, one frame per Gaussian) or "straddle" (a divisor whose group size N / F is not a
    multiple of 64, so that 64-lane units straddle two frames; F = N when N has none).  `pick` in [0, 1) chooses among the candidates."""
    if n <= 1 or kind == "one":
        return 1
    if kind == "each":
        return n
    cand = [f for f in range(2, n) if n % f == 0 and (n // f) % 64]
    return cand[int(pick * len(cand))] if cand else n


def draw_sr_case(rng, build: bool = True):
    """One random case of the scale / rotation form: -> (desc, inputs), inputs = (cfg, viewbuf, means, records, opac, colors, extra,
    g_color, g_extra, capacity, frames, sh_frame, want_views), CPU tensors; records (S, N, 7) = scale + un-normalised quaternion
    (x, y, z, w); frames None or (S, F, 3, 3) proper rotations, different in every set; cfg without the SH-frame bits (sh_frame names
    them: gpu_util.run_both adds them on the HIP side).  Every draw comes from `rng` before anything is built and the tensors come
    from the drawn seed, so build=False leaves the generator exactly where build=True does: -> (desc, None)."""
    n = int(rng.choice([0, 1, 7, 63, 64, 65, 500, 1023, 1024, 1025, 3000, 9000, 20000]))
    h, w = int(rng.integers(1, 161)), int(rng.integers(1, 161))
    if rng.random() < 0.15:
        h, w = int(rng.choice([8, 16, 64, 128])), int(rng.choice([8, 16, 64, 128]))
    sets = int(rng.choice([1, 2, 2, 3, 4]))
    vps = int(rng.choice([1, 2, 3]))
    views = sets * vps
    sh_frame = SR_SH_FRAMES[int(rng.integers(0, 3))]
    use_sh = bool(sh_frame is not None or rng.random() < 0.8)  # precomputed colours only without an SH frame
    deg = int(rng.integers(0, 5))
    d_sh = int(rng.integers(deg + 1, 6)) ** 2 if use_sh else 0  # at least (deg + 1)^2 coefficients
    max_sh_eval = int(rng.choice([3, 4]))
    planar = bool(use_sh and rng.random() < 0.5)
    with_frames = bool(sh_frame is not None or rng.random() < 0.7)
    frame_kind = str(rng.choice(["one", "each", "straddle", "straddle"]))
    f = _sr_frame_count(n, frame_kind, float(rng.random())) if with_frames else 0
    with_extra = bool(rng.random() < 0.6)
    emode = int(rng.integers(1, 5)) if (with_extra and rng.random() < 0.5) else 0
    windowed = bool(rng.random() < 0.2)
    follows = bool(rng.random() < 0.5)
    det = bool(rng.random() < 0.3)
    cap = None if rng.random() < 0.7 else int(rng.integers(1, 5000))
    want_views = (False, True, "depth")[int(rng.integers(0, 3))]
    nears = [float(rng.choice([1.0, 0.5, 2.0])) for _ in range(sets)]
    scale_inv = [bool(rng.random() < 0.7) for _ in range(sets)]
    seed = int(rng.integers(0, 1 << 30))
    desc = dict(n=n, hw=(h, w), sets=sets, vps=vps, sh_frame=sh_frame, use_sh=use_sh, deg=deg, d_sh=d_sh, max_sh_eval=max_sh_eval,
                planar=planar, frames=f, extra=with_extra, emode=emode, windowed=windowed, follows=follows, det=det, cap=cap,
                want_views=want_views, seed=seed)
    if not build:
        return desc, None
    g = torch.Generator().manual_seed(seed)
    scs = [synthetic.make_scene(seed + s, n, (h, w), num_views=vps, d_sh=1, near=nears[s]) for s in range(sets)]
    means = torch.cat([sc.gaussians.means for sc in scs], 0).contiguous()
    opac = torch.cat([sc.gaussians.opacities for sc in scs], 0).contiguous()
    vb = torch.cat([gpu_util.scene_viewbuf(sc, scale_inv[s]) for s, sc in enumerate(scs)], 0)
    # scales as tests/test_gpu_sh_frame.py sizes them: 0.5 .. 15 x (4 px at the image's width) at the Gaussian's distance
    scales = (0.5 + 14.5 * torch.rand((sets, n, 3), generator=g)) * means.norm(dim=-1, keepdim=True) * (4.0 / (0.86 * max(w, 16)))
    records = torch.cat((scales, torch.randn((sets, n, 4), generator=g)), -1).contiguous()
    if use_sh:
        colors = 0.4 * torch.randn((sets, n, 3, d_sh) if planar else (sets, n, d_sh, 3), generator=g)
    else:
        colors = torch.rand((sets, n, 3), generator=g)
    frames = None
    if f:
        q = torch.linalg.qr(torch.randn((sets, f, 3, 3), dtype=torch.float64, generator=g))[0]
        frames = (q * torch.det(q)[..., None, None]).float().contiguous()  # proper rotations, independent in every set
    extra = torch.rand((views, n), generator=g) * 1.5 + 0.5 if (with_extra and not emode) else None
    gc = torch.rand((views, 3, h, w), generator=g)
    ge = torch.rand((views, h, w), generator=g) if with_extra else None
    flags = (_lib.FLAG_WINDOWED_BINNING if windowed else 0) | (_lib.FLAG_SH_PLANAR if planar else 0) | (emode << 4) | \
        (_lib.FLAG_BACKWARD_FOLLOWS if follows else 0) | (_lib.FLAG_DETERMINISTIC if det else 0)
    cfg = RasterConfig(views, sets, vps, n, h, w, deg if use_sh else 0, d_sh, max_sh_eval, with_extra, flags, True)
    return desc, (cfg, vb, means, records, opac.contiguous(), colors.contiguous(), extra, gc, ge, cap, frames, sh_frame, want_views)


def named_sr_case(seed: int, index: int):
    """Case `index` of the scale / rotation sequence `np.random.default_rng(seed)` generates."""
    rng = np.random.default_rng(seed)
    for _ in range(index):
        draw_sr_case(rng, build=False)
    return draw_sr_case(rng, build=True)
