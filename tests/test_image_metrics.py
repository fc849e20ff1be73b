"""The evaluation metrics of the raster path from one launch pair (gsr_image_metrics + gsr_image_metrics_finish;
pf3plat_amd.losses.compute_ssim / compute_image_metrics): compute_ssim as scikit-image defines it - reflected borders, sample
covariance, the interior mean, per image - against its numpy restatement tests/skimage_ssim.py.  CPU: the restatement's filter
against scipy, every clause of the definition shown to matter at the scale of the GPU bar, the host side of the three C entry
points and the Python argument checks.  GPU: values and maps against the float64 restatement, the bar tied to what the SAME
restatement loses in float32."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import losses as oracle_losses
from tests import skimage_ssim
from tests.test_losses import make_images, out_of_range_images

KINDS = ("noise", "blobs", "flat", "equal", "grain")  # tests/test_losses.py's four, and the one on which cn = 121 / 120 shows
# (n, h, w): the smallest legal image (an interior of one pixel, every tap of both axes reflected); one axis minimal and the other
# across a tile edge; exactly one tile; tiles one pixel wide on both axes (their halo is all reflection); ragged; the decoder's
# size; 19 x 35 x 3 = 1995 slots in one image (the finish loop's second trip); many images
BIG, MANY = (1, 304, 560), (40, 24, 40)
SHAPES = [(1, 11, 11), (1, 11, 27), (1, 27, 11), (1, 16, 16), (1, 17, 33), (1, 100, 24), (1, 45, 70), (1, 256, 256), BIG, MANY]
K_OWN, SSIM_FLOOR = 4.0, 2e-5  # tests/test_losses.py: two 11-tap passes in another order have the same order of rounding, other bits
VALUE_CAP, MAP_CAP = 2e-4, 1e-3  # no case's bar may be wider than these: an input that needs more is a badly chosen input
ids = lambda s: "x".join(map(str, s))


def grain_images(n, h, w, seed=0):
    """0.5 +- 0.0212 z, z white noise: two opposite images of local variance C2 / 2.  With covariance -v, S is about
    (C2 - 2 cn v) / (C2 + 2 cn v), whose derivative in cn, -4 v C2 / (C2 + 2 cn v)^2, is largest (1 / 2) at v = C2 / 2: the
    metric's cn = 121 / 120 moves the value by some 4e-3, the most a single image can show of it."""
    g = torch.Generator().manual_seed(15485863 * seed + 29)
    z = 0.0212 * torch.randn((n, 3, h, w), generator=g, dtype=torch.float64)
    return (0.5 - z).to(torch.float32), (0.5 + z).to(torch.float32)


@functools.lru_cache(maxsize=None)
def reference(kind, shape):
    """-> (prediction, ground truth) float32 torch, (values, maps) of the restatement in float64 and in float32; computed once per
    case and shared (nobody writes into it)."""
    build = {"out_of_range": out_of_range_images, "grain": grain_images}.get(kind) or functools.partial(make_images, kind)
    pred, target = build(*shape)
    gt, hat = target.numpy(), pred.numpy()
    return pred, target, skimage_ssim.structural_similarity(gt, hat, np.float64), skimage_ssim.structural_similarity(gt, hat, np.float32)


def value_bar(kind, shape):
    _, _, (v64, _), (v32, _) = reference(kind, shape)
    assert v32.dtype == np.float32 and v64.dtype == np.float64
    return np.maximum(SSIM_FLOOR, K_OWN * np.abs(v32.astype(np.float64) - v64))  # per image


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_restated_filter_is_scipys_reflecting_gaussian_filter():
    ndimage = pytest.importorskip("scipy.ndimage")
    img = np.random.default_rng(3).random((17, 33))
    want = ndimage.gaussian_filter(img, sigma=1.5, truncate=3.5, mode="reflect")
    got = skimage_ssim.gaussian_filter(img, np.float64)
    print(f"[metrics] filter vs scipy: {np.abs(got - want).max():.1e}")
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-14
    assert np.abs(skimage_ssim.gaussian_filter(img, np.float64, reflect=False) - want).max() > 1e-2  # zero padding is another filter


def test_metric_is_not_the_loss_ssim_and_every_clause_of_its_definition_is_load_bearing():
    """On the seeded 24 x 40 images, in float64 and in units of the GPU bar of the same case (figures: docs/PARITY.md):
      * noise: the metric and the loss's SSIM (oracle/losses.py: zero padding, population covariance, mean over every pixel) are
        269 bars apart;
      * reflection replaced by zero padding: the VALUE does not move at all - every tap of an interior pixel lies inside the image,
        which is why scikit-image crops - so the boundary clause bears on the map alone, and there by thousands of map bars;
      * the crop dropped: 83 bars on noise, more than 1000 on `grain`;
      * cn = 1: 0.1 bar on noise (cn scales numerator and denominator alike wherever the variances dwarf C2), 1 to 3 bars on blobs
        and flat; `grain` - two opposite images whose local variance is C2 / 2, where d S / d cn is largest - is the input on
        which the sample covariance is visible: about 200 bars.
    Each clause is asserted at 100 bars on the case where it acts; the GPU tests run all of these kinds."""
    shape = (1, 24, 40)

    def apart(kind, **switch):
        pred, target, (v64, m64), (_, m32) = reference(kind, shape)
        bar, mbar = float(value_bar(kind, shape)[0]), max(SSIM_FLOOR, K_OWN * np.abs(m32.astype(np.float64) - m64).max())
        assert bar <= VALUE_CAP and mbar <= MAP_CAP
        v, m = skimage_ssim.structural_similarity(target.numpy(), pred.numpy(), np.float64, **switch)
        dv, dm = abs(v[0] - v64[0]) / bar, np.abs(m - m64).max() / mbar
        print(f"[metrics] {kind:6s} 1x24x40 {str(switch):30s} value moves {dv:8.1f} bars   map moves {dm:8.1f} map bars")
        return dv, dm

    pred, target, (v64, _), _ = reference("noise", shape)
    loss_ssim = oracle_losses.ssim_map(pred.double(), target.double()).mean().item()
    print(f"[metrics] noise  1x24x40 metric {v64[0]:.6f}   the loss's SSIM {loss_ssim:.6f}")
    assert abs(loss_ssim - v64[0]) > 100 * float(value_bar("noise", shape)[0])
    figures = {(kind, name): apart(kind, **switch) for kind in ("noise", "blobs", "flat", "grain")
               for name, switch in (("zero padding", {"reflect": False}), ("no crop", {"crop": False}), ("cn = 1", {"sample_covariance": False}))}
    for kind in ("noise", "blobs", "flat", "grain"):
        assert figures[kind, "zero padding"][0] == 0 and figures[kind, "no crop"][1] == 0
    assert figures["noise", "zero padding"][1] > 100 and figures["grain", "zero padding"][1] > 100
    assert figures["grain", "no crop"][0] > 100
    assert figures["grain", "cn = 1"][0] > 100
    # symmetric in its arguments, 1 on equal images, and the restatement refuses what scikit-image refuses
    gt, hat = target.numpy(), pred.numpy()
    assert abs(skimage_ssim.structural_similarity(hat, gt, np.float64)[0][0] - v64[0]) < 1e-14
    ones, ones_map = skimage_ssim.structural_similarity(gt, gt, np.float32)
    assert np.all(ones == 1) and np.all(ones_map == 1)
    with pytest.raises(ValueError, match="win_size exceeds image extent"):
        skimage_ssim.structural_similarity(gt[:, :, :10], hat[:, :, :10])


def test_bars_of_the_gpu_cases_stay_under_their_caps():
    """The conditions of the GPU tests, checked without one on the small shapes: max(2e-5, 4 |f32 - f64|) <= 2e-4 per image,
    max(2e-5, 4 max |f32 - f64|) <= 1e-3 per map."""
    for kind in KINDS:
        for shape in SHAPES[:7]:
            _, _, (_, m64), (_, m32) = reference(kind, shape)
            vbar, mbar = value_bar(kind, shape).max(), max(SSIM_FLOOR, K_OWN * np.abs(m32.astype(np.float64) - m64).max())
            print(f"[metrics] {kind:6s} {ids(shape):10s} value bar {vbar:.2e}   map bar {mbar:.2e}")
            assert vbar <= VALUE_CAP and mbar <= MAP_CAP, (kind, shape, vbar, mbar)


def test_image_metrics_partials_count_argument_checks_and_exports():
    """Host side of the three entry points, no launch (here there is no device: a call that got past its checks would return the
    launch error instead): the slot count, 0 / GSR_ERR_INVALID_ARGUMENT for what the launch refuses, GSR_OK for an empty batch; the
    additions leave the ABI version at 5."""
    from pf3plat_amd import _lib

    lib = _lib.load()
    assert lib.gsr_abi_version() == 5 == _lib.GSR_ABI_VERSION
    exported = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    for name in ("gsr_image_metrics", "gsr_image_metrics_partials", "gsr_image_metrics_finish"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(exported, name) and f"{name}(" in header, name
    invalid = -1  # GSR_ERR_INVALID_ARGUMENT of include/gsr.h
    for n, h, w in SHAPES + [(2, BIG[1], BIG[2]), (6, 256, 256), (3, 33, 21), (21845, 11, 11)]:
        assert lib.gsr_image_metrics_partials(n, h, w) == n * 3 * -(-h // 16) * -(-w // 16) == lib.gsr_image_loss_partials(n, h, w), (n, h, w)
    assert lib.gsr_image_metrics_partials(*BIG) == 1995 > 1024
    for bad in ((0, 16, 16), (-1, 16, 16), (1, 10, 16), (1, 16, 10), (1, 0, 16), (1, 16, -5), (1, 1, 1), (0, 0, 0), (21846, 16, 16)):
        assert lib.gsr_image_metrics_partials(*bad) == 0, bad
    p = ctypes.c_void_p(4096)  # a non-null address that is never read: every call below returns before its launch
    run = lambda n, h, w, gt=p, pred=p, smap=p, part=p: lib.gsr_image_metrics(n, h, w, gt, pred, smap, part, None)
    for n, h, w in ((1, 10, 16), (1, 16, 10), (1, 0, 16), (1, 16, -1), (-1, 16, 16), (0, 10, 16), (0, 16, 10)):
        assert run(n, h, w) == invalid, (n, h, w)
    assert run(0, 16, 16) == 0 and run(0, 11, 11, None, None, None, None) == 0
    assert run(1, 16, 16, gt=None) == invalid and run(1, 16, 16, pred=None) == invalid and run(1, 16, 16, part=None) == invalid
    assert run(21846, 16, 16) == invalid and run(1 << 30, 16, 16) == invalid  # 3 n > 65535: more than a grid's z extent
    finish = lambda n, h, w, part=p, out=p: lib.gsr_image_metrics_finish(n, h, w, part, out, None)
    for n, h, w in ((0, 16, 16), (-1, 16, 16), (1, 10, 16), (1, 16, 10), (21846, 16, 16)):
        assert finish(n, h, w) == invalid, (n, h, w)
    assert finish(1, 16, 16, part=None) == invalid and finish(1, 16, 16, out=None) == invalid


def test_metrics_refuse_cpu_tensors_small_images_and_other_shapes(monkeypatch):
    """ValueError for a side below 11 (scikit-image's words) and for anything but two equal (n, 3, h, w) shapes - decided from the
    shapes alone, before the device is looked at and before the library is loaded; RuntimeError for CPU tensors of a legal shape."""
    from pf3plat_amd import _lib, losses

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    z = lambda *s: torch.zeros(s)
    for fn in (losses.compute_ssim, losses.compute_image_metrics):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(z(1, 3, 16, 16), z(1, 3, 16, 16))
        for h, w in ((10, 16), (16, 10), (1, 1)):
            with pytest.raises(ValueError, match="win_size exceeds image extent"):
                fn(z(2, 3, h, w), z(2, 3, h, w))
        with pytest.raises(ValueError, match="win_size exceeds image extent"):
            fn(z(0, 3, 10, 16), z(0, 3, 10, 16))
        for a, b in ((z(1, 3, 16, 16), z(1, 3, 16, 17)), (z(1, 3, 16, 16), z(2, 3, 16, 16)), (z(3, 16, 16), z(3, 16, 16)),
                     (z(1, 1, 16, 16), z(1, 1, 16, 16)), (z(1, 16, 16, 3), z(1, 16, 16, 3))):
            with pytest.raises(ValueError, match=r"\(n, 3, h, w\)"):
                fn(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.compute_image_metrics(z(1, 3, 16, 16), z(1, 3, 16, 16), ssim_map=True)


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_hip_ssim_values_against_float64_restatement(kind, shape):
    """Per image |hip - f64| <= max(2e-5, 4 |f32 - f64|), no bar above 2e-4; `equal`: within 1e-6 of 1."""
    from pf3plat_amd import losses

    pred, target, (v64, _), (v32, _) = reference(kind, shape)
    got = losses.compute_ssim(target.to(DEV), pred.to(DEV))
    assert got.shape == (shape[0],) and got.dtype == torch.float32 and got.device == torch.device(DEV)
    got = got.double().cpu().numpy()
    if kind == "equal":
        print(f"[metrics] {kind:6s} {ids(shape):10s} max |hip - 1|: {np.abs(got - 1).max():.1e}")
        assert np.all(np.abs(got - 1) <= 1e-6)
        return
    bar, err = value_bar(kind, shape), np.abs(got - v64)
    k = int((err / bar).argmax())
    print(f"[metrics] {kind:6s} {ids(shape):10s} value   hip vs float64: {err[k]:.3e}   float32 restatement vs float64: "
          f"{abs(float(v32[k]) - v64[k]):.3e}   bar: {bar[k]:.3e}   (image {k}; widest bar {bar.max():.3e})")
    assert bar.max() <= VALUE_CAP, (kind, shape, bar.max())
    assert np.all(np.isfinite(got)) and np.all(err <= bar), (kind, shape, k, err[k], bar[k])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_hip_ssim_map_against_float64_restatement(kind, shape):
    """Every pixel of the map, border included: max |hip - f64| <= max(2e-5, 4 max |f32 - f64|), no bar above 1e-3; the check that
    locates a wrong reflected index or a wrong tile seam.  The values that come with the map are those without it, bit for bit."""
    from pf3plat_amd import losses

    pred, target, (_, m64), (_, m32) = reference(kind, shape)
    gt, hat = target.to(DEV), pred.to(DEV)
    psnr, value, smap = losses.compute_image_metrics(gt, hat, ssim_map=True)
    assert smap.shape == (shape[0], 3) + shape[1:] and smap.dtype == torch.float32 and psnr.shape == value.shape == (shape[0],)
    assert torch.equal(value, losses.compute_ssim(gt, hat))
    smap = smap.double().cpu().numpy()
    if kind == "equal":
        assert np.all(np.abs(smap - 1) <= 1e-6) and torch.all(torch.isposinf(psnr))
        return
    own, err = np.abs(m32.astype(np.float64) - m64).max(), np.abs(smap - m64)
    bar = max(SSIM_FLOOR, K_OWN * own)
    at = np.unravel_index(err.argmax(), err.shape)
    print(f"[metrics] {kind:6s} {ids(shape):10s} map     hip vs float64: {err.max():.3e} at {at}   float32 restatement vs float64: {own:.3e}   bar: {bar:.3e}")
    assert bar <= MAP_CAP, (kind, shape, bar)
    assert np.all(np.isfinite(smap)) and err.max() <= bar, (kind, shape, at, err.max(), bar)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 45, 70), MANY], ids=ids)
def test_hip_psnr_from_the_metrics_launch_with_values_outside_0_1(shape):
    """Inputs from -0.3 to 1.3, so the clip of compute_psnr acts: the PSNR of the metrics launch against the oracle's in float64 and
    against the existing compute_psnr, rtol 1e-5; the SSIM of the same launch sees the unclipped values."""
    from pf3plat_amd import losses

    pred, target, (v64, _), _ = reference("out_of_range", shape)
    gt, hat = target.to(DEV), pred.to(DEV)
    psnr, value = losses.compute_image_metrics(gt, hat)
    want = oracle_losses.psnr(target.double(), pred.double()).numpy()
    got = psnr.double().cpu().numpy()
    print(f"[metrics] out of range {ids(shape):10s} psnr hip vs float64: {np.abs(got / want - 1).max():.3e} (relative)")
    np.testing.assert_allclose(got, want, rtol=1e-5)
    np.testing.assert_allclose(got, losses.compute_psnr(gt, hat).double().cpu().numpy(), rtol=1e-5)
    bar = value_bar("out_of_range", shape)
    assert bar.max() <= VALUE_CAP and np.all(np.abs(value.double().cpu().numpy() - v64) <= bar)


@pytest.mark.gpu
def test_hip_metrics_repeat_batch_and_input_forms_give_the_same_bits():
    """Two runs; every image of the 40-image batch against its own single-image call; float64 and channel-strided inputs against
    their float32 contiguous copies; compute_ssim against compute_image_metrics: the same bits each time (no atomics, fixed order,
    an image's sums independent of the rest of the batch).  An empty batch gives empty results."""
    from pf3plat_amd import losses

    pred, target, _, _ = reference("noise", MANY)
    gt, hat = target.to(DEV), pred.to(DEV)
    a, b = losses.compute_image_metrics(gt, hat, ssim_map=True), losses.compute_image_metrics(gt, hat, ssim_map=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    plain = losses.compute_image_metrics(gt, hat)
    assert len(plain) == 2 and torch.equal(plain[0], a[0]) and torch.equal(plain[1], a[1]) and torch.equal(losses.compute_ssim(gt, hat), a[1])
    for i in range(MANY[0]):
        one = losses.compute_image_metrics(gt[i:i + 1], hat[i:i + 1], ssim_map=True)
        assert torch.equal(one[0], a[0][i:i + 1]) and torch.equal(one[1], a[1][i:i + 1]) and torch.equal(one[2], a[2][i:i + 1]), i
    big_pred, big_target, _, _ = reference("blobs", BIG)
    x, y = losses.compute_image_metrics(big_target.to(DEV), big_pred.to(DEV)), losses.compute_image_metrics(big_target.to(DEV), big_pred.to(DEV))
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    nhwc = pred.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)  # channel-strided
    wide = torch.full((MANY[0], 3, MANY[1], 2 * MANY[2]), 7.0)
    wide[..., ::2] = target
    sliced = wide.to(DEV)[..., ::2]
    assert not nhwc.is_contiguous() and not sliced.is_contiguous()
    for g, h in ((gt, nhwc), (sliced, hat), (gt.double(), hat.double()), (sliced.double(), nhwc)):
        out = losses.compute_image_metrics(g, h, ssim_map=True)
        assert all(o.dtype == torch.float32 and torch.equal(o, r) for o, r in zip(out, a))
        assert torch.equal(losses.compute_ssim(g, h), a[1])
    empty = torch.zeros((0, 3, 24, 40), device=DEV)
    psnr, value, smap = losses.compute_image_metrics(empty, empty, ssim_map=True)
    assert psnr.shape == value.shape == (0,) and smap.shape == (0, 3, 24, 40) and losses.compute_ssim(empty, empty).shape == (0,)
