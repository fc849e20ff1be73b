"""`-m gpu`: the small kernels beside the raster path, each against a plain float64 restatement at the sizes where a one-thread-per-
item kernel goes wrong (one item, a block edge on either side, many blocks): covariance from scale + quaternion and its backward
(k_cov_from_scale_rot[_bwd]), the visibility mask (k_mark_visible: per-set camera, per-view scale, the near-plane decision) and the
camera records (k_setup_views, k_setup_views_ortho, k_setup_views_bwd).  Measured distances: docs/PARITY.md, "small ops"."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import cameras
from pf3plat_amd import _lib, rasterizer
from pf3plat_amd.rasterizer import RasterConfig
from tests.oracle_backend import OracleBackend
from tests.util import look_at_c2w, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_OWN = 4.0  # bar = max(floor, 4 x what the same formula loses in float32 torch on the CPU): same order of rounding, other bits
COV_FLOOR = 1e-5  # the conic bound of tests/parity_checks.py
TINY = 1e-30


# --------------------------------------------------------------------------------------------------------------------------
# covariance from scale and rotation
# --------------------------------------------------------------------------------------------------------------------------
def cov_inputs(n, seed=0, zero_row=True):
    """Scales log-uniform over 1e-3 .. 1e2 per axis; quaternions (r, x, y, z) randn, NOT normalised, norms log-uniform over 0.1 .. 10,
    one all-zero row in the middle; dL/dcov6 randn with row sizes log-uniform over 1e-2 .. 1e2.  float32, CPU."""
    g = torch.Generator().manual_seed(31 * seed + n % 1009)
    f64 = torch.float64
    scales = 10 ** (-3 + 5 * torch.rand((n, 3), generator=g, dtype=f64))
    q = torch.randn((n, 4), generator=g, dtype=f64)
    q = q / q.norm(dim=1, keepdim=True) * 10 ** (-1 + 2 * torch.rand((n, 1), generator=g, dtype=f64))
    if zero_row:
        q[n // 2] = 0
    d_cov6 = torch.randn((n, 6), generator=g, dtype=f64) * 10 ** (-2 + 4 * torch.rand((n, 1), generator=g, dtype=f64))
    return scales.float(), q.float(), d_cov6.float()


def cov_reference(scales, rots, mod, d_cov6, dtype):
    """Sigma = R diag((m s)^2) R^T in `dtype` torch on the CPU, R from (r, x, y, z) without normalisation, entries in the order
    xx, xy, xz, yy, yz, zz; gradients by autograd of <dSigma, Sigma> over the full 3 x 3 matrix.  The incoming dL/dcov6 follows the
    rasterizer backward's convention - an off-diagonal entry holds the SUM of the two symmetric partials - so the symmetric dSigma
    gets HALF of it at (i, j) and half at (j, i)."""
    s, q = scales.detach().clone().to(dtype).requires_grad_(True), rots.detach().clone().to(dtype).requires_grad_(True)
    r, x, y, z = q.unbind(-1)
    rm = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                      2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)), -1).reshape(-1, 3, 3)
    sc = mod * s
    sigma = rm @ torch.diag_embed(sc * sc) @ rm.transpose(1, 2)
    d = d_cov6.to(dtype)
    d_sigma = torch.stack((d[:, 0], 0.5 * d[:, 1], 0.5 * d[:, 2],
                           0.5 * d[:, 1], d[:, 3], 0.5 * d[:, 4],
                           0.5 * d[:, 2], 0.5 * d[:, 4], d[:, 5]), -1).reshape(-1, 3, 3)
    d_s, d_q = torch.autograd.grad((sigma * d_sigma).sum(), (s, q))
    cov6 = torch.stack((sigma[:, 0, 0], sigma[:, 0, 1], sigma[:, 0, 2], sigma[:, 1, 1], sigma[:, 1, 2], sigma[:, 2, 2]), -1)
    return [t.detach().double().numpy() for t in (cov6, d_s, d_q)]


def row_error(got, want):
    """Per Gaussian, against the row's own size: |got - want|_inf / (|want row|_inf + tiny), worst row.  (A rel-L2 over all rows would
    let the scales near 1e2 hide the ones near 1e-3.)"""
    err = np.abs(got - want).max(1) / (np.abs(want).max(1) + TINY)
    return float(err.max()), int(err.argmax())


@pytest.mark.parametrize("mod", [1.0, 1.5, 0.25])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 200_003])
def test_cov_from_scale_rot_forward_and_backward_against_float64(n, mod):
    scales, rots, d_cov6 = cov_inputs(n, zero_row=n > 1)
    be = rasterizer.get_backend()
    cov6 = be.cov_from_scale_rot(scales.to(DEV), rots.to(DEV), mod)
    d_s, d_q = be.cov_from_scale_rot_backward(scales.to(DEV), rots.to(DEV), mod, d_cov6.to(DEV))
    assert cov6.shape == (n, 6) and d_s.shape == (n, 3) and d_q.shape == (n, 4)
    got = [t.double().cpu().numpy() for t in (cov6, d_s, d_q)]
    want, f32 = cov_reference(scales, rots, mod, d_cov6, torch.float64), cov_reference(scales, rots, mod, d_cov6, torch.float32)
    rows = []
    for name, a, w, o in zip(("cov6", "d_scales", "d_rotations"), got, want, f32):
        assert np.isfinite(a).all(), name
        (err, at), (own, _) = row_error(a, w), row_error(o, w)
        rows.append((name, err, at, max(COV_FLOOR, K_OWN * own)))
        print(f"[small ops] cov n={n:<6d} mod={mod:<4} {name:11s} hip vs float64: {err:.3e}   float32 torch vs float64: {own:.3e}   bar: {rows[-1][3]:.3e}")
    for name, err, at, bar in rows:
        assert err <= bar, (name, n, mod, err, bar, at)
    if n > 1:  # the all-zero quaternion: R = I, Sigma = diag((m s)^2), dL/dq = 0 and dL/ds_k = 2 m^2 s_k dSigma_kk
        z = n // 2
        ms2 = (mod * scales[z].double().numpy()) ** 2
        np.testing.assert_allclose(got[0][z], [ms2[0], 0, 0, ms2[1], 0, ms2[2]], rtol=1e-6, atol=0)
        assert np.all(got[2][z] == 0) and np.all(want[2][z] == 0)
        np.testing.assert_allclose(got[1][z], want[1][z], rtol=1e-6, atol=0)


def test_cov_from_scale_rot_single_all_zero_quaternion():
    scales, _, d_cov6 = cov_inputs(1, seed=3, zero_row=False)
    rots = torch.zeros((1, 4))
    be = rasterizer.get_backend()
    for mod in (1.0, 1.5):
        cov6 = be.cov_from_scale_rot(scales.to(DEV), rots.to(DEV), mod).double().cpu().numpy()
        d_s, d_q = (t.double().cpu().numpy() for t in be.cov_from_scale_rot_backward(scales.to(DEV), rots.to(DEV), mod, d_cov6.to(DEV)))
        want = cov_reference(scales, rots, mod, d_cov6, torch.float64)
        ms2 = (mod * scales[0].double().numpy()) ** 2
        np.testing.assert_allclose(cov6[0], [ms2[0], 0, 0, ms2[1], 0, ms2[2]], rtol=1e-6, atol=0)
        np.testing.assert_allclose(cov6, want[0], rtol=1e-6, atol=0)
        np.testing.assert_allclose(d_s, want[1], rtol=1e-6, atol=0)
        assert np.all(d_q == 0) and np.all(want[2] == 0)


@pytest.mark.parametrize("n", [1, 257, 1000])
def test_cov_backward_writes_only_the_outputs_it_is_given(n):
    """The C entry point takes a null dL_dscales or dL_drotations and the kernel branches on each: the output that is asked for holds
    the bits of the call with both, and the memory around it - where the other one would lie - keeps what was there."""
    lib = _lib.load()
    scales, rots, d_cov6 = (t.to(DEV) for t in cov_inputs(n, seed=1))
    mod = 1.5
    both_s, both_r = rasterizer.get_backend().cov_from_scale_rot_backward(scales, rots, mod, d_cov6)
    stream = rasterizer._stream_ptr(torch.device(DEV))
    sentinel = -12345.0

    def call(want_s, want_r):
        # one block: [guard | d_scales | guard | d_rotations | guard]
        block = torch.full((16 + 3 * n + 16 + 4 * n + 16,), sentinel, device=DEV)
        ds, dr = block[16:16 + 3 * n], block[32 + 3 * n:32 + 7 * n]
        rc = lib.gsr_cov_from_scale_rot_backward(n, scales.data_ptr(), rots.data_ptr(), ctypes.c_float(mod), d_cov6.data_ptr(),
                                                 ds.data_ptr() if want_s else None, dr.data_ptr() if want_r else None, stream)
        assert rc == 0
        torch.cuda.synchronize()
        guards = torch.cat((block[:16], block[16 + 3 * n:32 + 3 * n], block[32 + 7 * n:]))
        assert torch.all(guards == sentinel)
        return ds.reshape(n, 3), dr.reshape(n, 4)

    ds, dr = call(True, True)
    assert torch.equal(ds, both_s) and torch.equal(dr, both_r)
    ds, dr = call(False, True)
    assert torch.all(ds == sentinel) and torch.equal(dr, both_r)
    ds, dr = call(True, False)
    assert torch.equal(ds, both_s) and torch.all(dr == sentinel)
    ds, dr = call(False, False)
    assert torch.all(ds == sentinel) and torch.all(dr == sentinel)


# --------------------------------------------------------------------------------------------------------------------------
# mark_visible
# --------------------------------------------------------------------------------------------------------------------------
def near_threshold_from_source():
    """kNear of pf3plat_amd/csrc/gsr_common.h: `present = !(camera depth <= kNear)`, the forward's cull (in_frustum) with the same constant."""
    src = open(os.path.join(os.path.dirname(_lib.SRC), "gsr_common.h")).read()
    (value,) = re.findall(r"constexpr float kNear = ([0-9.]+)f;", src)
    return np.float32(value)


SETS, VIEWS_PER_SET = 3, 2
ULP_STEPS = (-16, -8, -3, -1, 0, 1, 3, 8, 16)  # placed depths: kNear + k ulp; |k| <= 3 may go either way in float32, 8 and 16 may not
BAND = 4


def visibility_case(n, k_near):
    """Six rotated cameras (set s reads record 2 s), each with its own near and therefore its own scale 1 / near, each at 0.2 x near
    from the world origin and looking at it: the near threshold of every camera passes through the origin, where float32 coordinates
    are fine enough to place a depth to a fraction of an ulp of kNear.  Point i of set s: (i + s) % 3 = 0 in front, 1 behind, 2 at the
    threshold (the first 54 of those; later ones alternate in front / behind).  "At the threshold" is kNear + k ulp for k in ULP_STEPS;
    the k = 0 point is ON the threshold as closely as a float32 mean allows - its float64 depth lands within about 1e-10 (a hundredth
    of an ulp of kNear) of it, on either side, not exactly on it - and like the other |k| <= 3 points it lies in the band.
    -> records (6, 48), means (S, n, 3) float32, float64 depths (S, n), the index lists of the threshold points."""
    rng = np.random.default_rng(1000 + n)
    nears = np.array([0.5, 2.9, 1.3, 0.8, 2.1, 3.7], np.float32)
    eyes = np.array([[0.3, -0.5, -1.0], [-1.0, 0.2, 0.4], [0.6, 0.7, -0.3], [-0.2, -0.9, 0.5], [0.9, -0.1, 0.8], [-0.5, 0.6, -0.7]])
    eyes = eyes / np.linalg.norm(eyes, axis=1, keepdims=True) * float(k_near) * nears[:, None].astype(np.float64)
    ext = np.stack([look_at_c2w(e, target=(0, 0, 0), up=u) for e, u in zip(eyes, [(0, -1, 0), (1, 0, 0), (0, 0, 1), (0, 1, 0.3), (0.2, 0, -1), (1, 1, 0)])])
    intr = np.tile(np.array([[0.8, 0, 0.5], [0, 0.9, 0.5], [0, 0, 1]], np.float32), (6, 1, 1))
    far = np.full(6, 100, np.float32)
    be = rasterizer.get_backend()
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(DEV)
    records = be.setup_views(t(ext), t(intr), t(nears), t(far), torch.zeros(3, device=DEV), True).cpu()
    rec = records.double().numpy()
    ulp = float(np.spacing(k_near))
    means = np.zeros((SETS, n, 3), np.float32)
    depth = np.zeros((SETS, n))
    placed = []
    for s in range(SETS):
        r = rec[s * VIEWS_PER_SET]
        row, tz, scale = r[[2, 6, 10]], r[14], r[40]  # depth(m) = scale (row . m) + tz, from the record the kernel reads
        kind = (np.arange(n) + s) % 3
        at_threshold, rest = np.split(np.flatnonzero(kind == 2), [6 * len(ULP_STEPS)])
        kind[rest] = rng.integers(0, 2, len(rest))
        target = np.where(kind == 0, float(k_near) + rng.uniform(0.05, 3.0, n), float(k_near) - rng.uniform(0.05, 3.0, n))
        start = rng.normal(size=(n, 3))
        start[at_threshold] *= 1e-3
        target[at_threshold] = float(k_near) + np.array(ULP_STEPS)[np.arange(len(at_threshold)) % len(ULP_STEPS)] * ulp
        m = start + ((target - (scale * (start @ row) + tz)) / scale)[:, None] * row[None] / (row @ row)
        means[s] = m.astype(np.float32)
        depth[s] = scale * (means[s].astype(np.float64) @ row) + tz
        placed.append(at_threshold)
    return records, torch.from_numpy(means), depth, placed


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_mark_visible_per_set_cameras_scale_and_near_plane(n):
    """present[s, i] == (scale_s (R_s m + t_s)_z > kNear) in float64 from the records of view 2 s, for every point further than 4 float32
    ulp from the threshold; the points inside that band are exactly the ones placed there and are counted; the oracle backend, which
    evaluates the kernel's own float32 expression in the kernel's order (the library is built without FMA contraction), gives the
    same mask for EVERY point, the band included; the three sets, fed the SAME means, give three different masks."""
    k_near = near_threshold_from_source()
    assert k_near == np.float32(0.2)
    records, means, depth, placed = visibility_case(n, k_near)
    cfg = RasterConfig(SETS * VIEWS_PER_SET, SETS, VIEWS_PER_SET, n, 64, 64, 0, 0)
    be = rasterizer.get_backend()
    got = be.mark_visible(cfg, records.to(DEV), means.to(DEV)).cpu().numpy()
    assert got.shape == (SETS, n) and got.dtype == bool
    want = depth > float(k_near)
    band = np.abs(depth - float(k_near)) <= BAND * float(np.spacing(k_near))
    for s in range(SETS):
        inside = np.flatnonzero(band[s])
        expected_inside = [i for j, i in enumerate(placed[s]) if abs(ULP_STEPS[j % len(ULP_STEPS)]) <= 3]
        assert sorted(inside) == sorted(expected_inside), (s, inside, expected_inside)  # the band holds exactly the points put there
        assert np.array_equal(got[s][~band[s]], want[s][~band[s]]), (s, np.flatnonzero((got[s] != want[s]) & ~band[s]))
        if n >= 255:
            just_outside = [i for j, i in enumerate(placed[s]) if abs(ULP_STEPS[j % len(ULP_STEPS)]) >= 8]
            assert len(just_outside) >= 8 and want[s][just_outside].any() and not want[s][just_outside].all()
            assert want[s].any() and not want[s].all()
    ref = OracleBackend().mark_visible(cfg, records, means).numpy()
    assert np.array_equal(ref, got), np.argwhere(ref != got)
    print(f"[small ops] mark_visible n={n}: {int(band.sum())} of {band.size} points within {BAND} ulp of kNear = {float(k_near)!r}; "
          f"of those the kernel and float64 differ on {int((got != want)[band].sum())}")
    if n >= 255:  # the per-set camera is used: one point cloud, three masks
        same = means[1:2].expand(SETS, n, 3).contiguous()
        masks = be.mark_visible(cfg, records.to(DEV), same.to(DEV)).cpu().numpy()
        d = np.stack([records[2 * s, 40].item() * (same[s].double().numpy() @ records[2 * s, [2, 6, 10]].double().numpy()) + records[2 * s, 14].item()
                      for s in range(SETS)])
        clear = np.abs(d - float(k_near)) > 1e-4
        assert np.array_equal(masks[clear], (d > float(k_near))[clear])
        assert (masks[0] != masks[1]).sum() > n // 10 and (masks[1] != masks[2]).sum() > n // 10 and (masks[0] != masks[2]).sum() > n // 10
        # ... and it is the set's FIRST view: the mask of set 1 is not what view 1 (set 0's second camera) would give
        d_wrong = records[1, 40].item() * (means[1].double().numpy() @ records[1, [2, 6, 10]].double().numpy()) + records[1, 14].item()
        assert ((d_wrong > float(k_near)) != got[1]).sum() > n // 10


def test_mark_visible_nan_mean_is_present_as_in_the_forward_cull():
    """`!(depth <= kNear)` is true for a NaN depth: the kernel reports such a point as present, exactly as the forward's cull keeps it
    at this step (the same expression on the same constant; it is dropped a few lines later, by its non-finite screen position), and the oracle backend's
    `~(z <= 0.2)` agrees."""
    k_near = near_threshold_from_source()
    records, means, depth, _ = visibility_case(256, k_near)
    means = means.clone()
    nan_at = [(0, 3, 0), (1, 100, 1), (2, 255, 2)]
    for s, i, c in nan_at:
        means[s, i, c] = float("nan")
    cfg = RasterConfig(SETS * VIEWS_PER_SET, SETS, VIEWS_PER_SET, 256, 64, 64, 0, 0)
    got = rasterizer.get_backend().mark_visible(cfg, records.to(DEV), means.to(DEV)).cpu().numpy()
    ref = OracleBackend().mark_visible(cfg, records, means).numpy()
    for s, i, _ in nan_at:
        assert got[s, i] and ref[s, i]
    band = np.abs(depth - float(k_near)) <= BAND * float(np.spacing(k_near))
    keep = ~band
    for s, i, _ in nan_at:
        keep[s, i] = False
    assert np.array_equal(got[keep], (depth > float(k_near))[keep]) and np.array_equal(ref, got)


# --------------------------------------------------------------------------------------------------------------------------
# view set-up
# --------------------------------------------------------------------------------------------------------------------------
def camera_batch(v, seed):
    """V seeded random cameras in the manner of tests/test_gpu_api.py's V = 5 test (not those five): eyes drawn from a box of similar
    extent, looking at (0, 0, 5), off-centre principal points; with them nears, fars, backgrounds and orthographic widths / heights."""
    gen = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(v, generator=gen)
    eyes = torch.stack((u(-0.5, 0.7), u(0.0, 0.8), u(-1.6, 0.0)), 1).double().numpy()
    ext = torch.stack([torch.tensor(look_at_c2w(e)) for e in eyes])
    intr = torch.eye(3).repeat(v, 1, 1)
    intr[:, 0, 0], intr[:, 1, 1], intr[:, 0, 2], intr[:, 1, 2] = u(0.6, 1.1), u(0.6, 1.1), u(0.45, 0.55), 0.5
    return ext, intr, u(0.5, 2.5), u(50, 100), torch.rand((v, 3), generator=gen), u(4, 8), u(3, 7)


@pytest.mark.parametrize("v", [1, 64, 65, 300])
def test_setup_views_kernels_at_block_edges(v):
    """k_setup_views / k_setup_views_ortho run 64 views per workgroup: one view, one full workgroup, one more, several.  Against
    oracle/cameras.py at the tolerances of the V = 5 test in tests/test_gpu_api.py."""
    ext, intr, near, far, bg, width, height = camera_batch(v, 3 + v)
    be = rasterizer.get_backend()
    d = lambda *ts: [t.to(DEV) for t in ts]
    for si in (True, False):
        got = be.setup_views(*d(ext, intr, near, far, bg), si).cpu()
        want = cameras.view_records(ext.numpy(), intr.numpy(), near.numpy(), far.numpy(), bg.numpy(), si)
        assert got.shape == (v, 48)
        np.testing.assert_allclose(got.numpy(), want, rtol=2e-5, atol=2e-6)
    one_bg = be.setup_views(*d(ext, intr, near, far, bg[0]), True).cpu()
    assert torch.allclose(one_bg[:, 37:40], bg[0].expand(v, 3))
    for fov in (10.0, 0.1):
        got, dump = be.setup_views_orthographic(*d(ext, width, height, near, far, bg), fov)
        want, wdump = cameras.view_records_orthographic(ext.numpy(), width.numpy(), height.numpy(), near.numpy(), far.numpy(), bg.numpy(), fov)
        assert got.shape == (v, 48)
        # the tiny field of view makes distances ~1e3..1e5: compare relative to the size of each record's entries
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=1e-4 * np.abs(want).max())
        for k in ("extrinsics", "fov_x", "fov_y", "near", "far"):
            np.testing.assert_allclose(dump[k].cpu().numpy(), wdump[k], rtol=1e-5, atol=1e-6, err_msg=k)


@pytest.mark.parametrize("v", [1, 64, 65, 300])
def test_setup_views_backward_at_block_edges(v):
    """k_setup_views_bwd against the closed form in float64 torch (tests/oracle_backend.py), the bar of the V = 5 test in
    tests/test_gpu_parity.py - over all views and for every view on its own, so that one wrong view among 300 shows."""
    gen = torch.Generator().manual_seed(9 + v)
    ext = torch.eye(4).repeat(v, 1, 1)
    ext[:, :3, :3] = torch.linalg.qr(torch.randn((v, 3, 3), generator=gen))[0]
    ext[:, :3, 3] = torch.randn((v, 3), generator=gen)
    intr = torch.tensor([[0.8, 0, 0.5], [0, 0.9, 0.5], [0, 0, 1.0]]).repeat(v, 1, 1)
    near, far = 0.5 + torch.rand(v, generator=gen), 40 + 20 * torch.rand(v, generator=gen)
    dvw = torch.randn((v, 48), generator=gen)
    dvw[:, 35:] = 0
    be = rasterizer.get_backend()
    for scale_invariant in (True, False):
        vb_cpu = OracleBackend().setup_views(ext, intr, near, far, torch.zeros(3), scale_invariant)
        want = OracleBackend().setup_views_backward(vb_cpu, dvw).numpy()
        got = be.setup_views_backward(vb_cpu.to(DEV), dvw.to(DEV)).cpu().numpy()
        assert got.shape == (v, 4, 4)
        worst = max(rel_l2(got[i], want[i]) for i in range(v))
        print(f"[small ops] setup_views_backward V={v} scale_invariant={scale_invariant}: rel-L2 {rel_l2(got, want):.3e}, worst view {worst:.3e}")
        assert rel_l2(got, want) < 1e-6 and worst < 1e-6
