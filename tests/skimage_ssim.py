"""The evaluation metric compute_ssim (reference src/evaluation/metrics.py:36-52) restated in numpy:
skimage.metrics.structural_similarity(gt, hat, win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0) per image, as
include/gsr.h states it.  scikit-image itself is not importable where the suite runs, so this text - and scipy for the filter,
tests/test_image_metrics.py - is what the kernel is pinned to (docs/PARITY.md).  Every array is held in `dtype` - float32 as scikit-image runs on
float32 images, float64 as the arbiter - and the two sums that scipy and scikit-image take in double whatever the arrays' type (a
filter line's taps, the mean of the map) are taken in double here too.  The keyword switches exist for the ablations of the CPU tests:
each clause of the definition, turned off, moves the value by far more than the GPU tests' bar."""
import numpy as np

WIN, RADIUS, SIGMA = 11, 5, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(dtype=np.float64):
    """exp(-k^2 / (2 sigma^2)), k = -5..5 (truncate 3.5 x sigma 1.5 = 5.25 -> radius 5), normalised; computed in float64 as scipy does."""
    k = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    w = np.exp(-0.5 * k * k / SIGMA ** 2)
    return (w / w.sum()).astype(dtype)


def gaussian_filter(img, dtype=np.float64, reflect=True):
    """scipy.ndimage.gaussian_filter(img, sigma=1.5, truncate=3.5, mode="reflect") over the last two axes: two 11-tap passes, the
    image extended by reflection about its edge (numpy's "symmetric"; reflect=False: by zeros, the loss's boundary)."""
    w = window(np.float64)
    out = np.asarray(img, dtype=dtype)
    for axis in (out.ndim - 2, out.ndim - 1):
        pad = [(0, 0)] * out.ndim
        pad[axis] = (RADIUS, RADIUS)
        ext = np.pad(out, pad, mode="symmetric") if reflect else np.pad(out, pad, mode="constant")
        n = out.shape[axis]
        acc = np.zeros(out.shape, dtype=np.float64)  # scipy's correlate1d adds a line's taps up in double whatever the array's type
        for k in range(WIN):
            acc = acc + w[k] * np.take(ext, np.arange(k, k + n), axis=axis)
        out = acc.astype(dtype)  # ... and stores the pass in the array's type
    return out


def structural_similarity(ground_truth, predicted, dtype=np.float64, reflect=True, crop=True, sample_covariance=True):
    """ground_truth, predicted (n, 3, h, w), h, w >= 11 -> (values (n,), maps (n, 3, h, w)) in `dtype`."""
    x, y = np.asarray(ground_truth, dtype=dtype), np.asarray(predicted, dtype=dtype)
    if x.shape != y.shape or x.ndim != 4 or x.shape[1] != 3:
        raise ValueError(f"expected two (n, 3, h, w) images, got {x.shape} and {y.shape}")
    if x.shape[2] < WIN or x.shape[3] < WIN:
        raise ValueError("win_size exceeds image extent")
    blur = lambda a: gaussian_filter(a, dtype, reflect)
    cn = dtype(WIN * WIN / (WIN * WIN - 1.0)) if sample_covariance else dtype(1)
    c1, c2, two = dtype(C1), dtype(C2), dtype(2)
    ux, uy = blur(x), blur(y)
    vx = cn * (blur(x * x) - ux * ux)
    vy = cn * (blur(y * y) - uy * uy)
    vxy = cn * (blur(x * y) - ux * uy)
    s = ((two * ux * uy + c1) * (two * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    assert s.dtype == dtype
    inner = s[:, :, RADIUS:s.shape[2] - RADIUS, RADIUS:s.shape[3] - RADIUS] if crop else s
    # the mean of a channel's map accumulates in float64 whatever the map's dtype (scikit-image: crop(S, pad).mean(dtype=float64))
    # and is kept in `dtype`; then the mean of the three channels
    values = inner.mean(axis=(2, 3), dtype=np.float64).astype(dtype).mean(axis=1, dtype=np.float64).astype(dtype)
    return values, s
