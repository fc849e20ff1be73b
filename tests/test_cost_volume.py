"""The plane-sweep cost volume (pf3plat_amd.cost_volume; gsr_cost_volume / gsr_cost_volume_backward; definition: include/gsr.h).

Yardstick: the float64 restatement of tests/cost_volume_ref.py, itself pinned to the reference's own functions by the records of
tests/golden/cost_volume_fixtures.npz (make_cost_volume_fixtures.py).  Bars (docs/PARITY.md section 15, the convention of section 13):
per case and quantity the HIP result lies within max(FLOOR, 4 x |float32 restatement - float64 restatement|) rel-L2 of the float64
restatement; FLOOR is the worst the float32 restatement loses over all the cases below, measured on the CPU and rounded up in the
second digit (the `tiles` case sets both: value 2.685e-6, gradient 2.564e-6; the others lose 3.3e-7 .. 9.1e-7); no bar is above 1e-4."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from pf3plat_amd import _lib
from tests import cost_volume_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "cost_volume_fixtures.npz")
NEAR, WIDE = 0.02, 0.1  # the rigs: pose spread (radians per axis and units of translation) of tests/cost_volume_ref.build_case
# name: (seed, (b, v, c, h, w, D), spread)
CASES = {
    "v2": (11, (2, 2, 8, 6, 9, 5), NEAR),
    "v2_wide": (5, (2, 2, 8, 6, 9, 5), WIDE),
    "v3": (3, (1, 3, 5, 7, 4, 6), WIDE),
    "v4": (2, (2, 4, 3, 5, 5, 4), WIDE),
    "v4_near": (2, (2, 4, 3, 5, 5, 4), NEAR),
    "wide_c": (1, (1, 2, 130, 8, 8, 8), WIDE),      # C past one pass of a 64- or 128-channel chunk, and not a multiple of 4
    "two_passes": (4, (1, 2, 261, 4, 5, 3), NEAR),  # C past one 256-channel pass of a wave, and not a multiple of 4
    "tiles": (1, (1, 2, 16, 17, 33, 7), WIDE),      # 561 pixels: 36 forward workgroups of 16, the last one a single pixel; h != w
    "d1": (6, (1, 2, 4, 6, 6, 1), NEAR),
    "d_many": (1, (1, 2, 4, 6, 6, 130), WIDE),      # three blocks of 64 candidates, the last one of two
}
VALUE_FLOOR = 2.7e-6
GRAD_FLOOR = 2.6e-6
CAP = 1e-4
INVALID = -1  # GSR_ERR_INVALID_ARGUMENT of include/gsr.h


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case, its float64 volume and gradient, and what the float32 restatement loses against them (computed once, shared)."""
    seed, shape, spread = CASES[name]
    case = ref.build_case(seed, *shape, spread)
    return (case,) + _yardstick(case)


def _yardstick(case):
    c64, g64 = ref.value_and_grad(ref.cost_volume, case, torch.float64)
    c32, g32 = ref.value_and_grad(ref.cost_volume, case, torch.float32)
    return c64, g64, ref.rel_l2(c32, c64), ref.rel_l2(g32, g64)


def bars(loss_value, loss_grad):
    bv, bg = max(VALUE_FLOOR, 4 * loss_value), max(GRAD_FLOOR, 4 * loss_grad)
    assert bv <= CAP and bg <= CAP, (bv, bg)
    return bv, bg


def fixture_case(name):
    with np.load(FIXTURES) as fx:
        case = {k: torch.from_numpy(fx[f"{name}.{k}"]) for k in ("features", "intrinsics", "extrinsics", "near", "far", "cotangent")}
        case["num"] = int(fx[f"{name}.num"])
        return case, torch.from_numpy(fx[f"{name}.cost"]), torch.from_numpy(fx[f"{name}.grad_features"])


# ---- without a GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v2", "v3"])
def test_restatement_reproduces_the_reference_record(name):
    case, cost, grad = fixture_case(name)
    seed, shape, spread = CASES[name]
    again = ref.build_case(seed, *shape, spread)
    for k in ("features", "intrinsics", "extrinsics", "near", "far", "cotangent"):
        assert torch.equal(case[k], again[k]), k  # the record is of the case the GPU tests run
    c64, g64 = ref.value_and_grad(ref.cost_volume, case, torch.float64)
    dv, dg = ref.rel_l2(cost, c64), ref.rel_l2(grad, g64)
    print(f"{name}: record vs float64 restatement: value {dv:.2e}, gradient {dg:.2e}")
    assert cost.dtype == torch.float32 and tuple(cost.shape) == (shape[1] * shape[0], shape[5], shape[3], shape[4])
    assert dv < 2e-5 and dg < 2e-5


@pytest.mark.parametrize("name", list(CASES))
def test_torch_form_equals_the_restatement_in_float64(name):
    case, c64, g64, _, _ = reference(name)
    t64, tg64 = ref.value_and_grad(ref.cost_volume_torch_form, case, torch.float64)
    assert ref.rel_l2(t64, c64) < 1e-12 and ref.rel_l2(tg64, g64) < 1e-12


@pytest.mark.parametrize("name", list(CASES))
def test_cases_exercise_what_they_claim(name):
    """Conditions on the float64 volume: a near rig has at most 10 % of it exactly zero (samples land inside), a wide rig between 20 %
    and 80 % (whole walks and parts of walks leave the image).  What the float32 restatement loses - the source of the floors - is printed."""
    case, c64, g64, lv, lg = reference(name)
    seed, (b, v, c, h, w, d), spread = CASES[name]
    assert tuple(c64.shape) == (v * b, d, h, w) and tuple(g64.shape) == (b, v, c, h, w)
    share = float((c64 == 0).double().mean())
    print(f"{name}: zero share {share:.3f}, float32 restatement loses value {lv:.2e}, gradient {lg:.2e}")
    if spread == NEAR:
        assert share <= 0.10, share
    else:
        assert 0.20 <= share <= 0.80, share
    assert float(g64.abs().max()) > 0
    bars(lv, lg)


def test_depth_candidates_are_the_references():
    from pf3plat_amd.cost_volume import depth_candidates

    case = reference("v2")[0]
    got = depth_candidates(case["near"], case["far"], 5)
    b, v = case["near"].shape
    assert got.shape == (v * b, 5) and got.dtype == torch.float32
    want = 1.0 / ref.candidates(case["near"], case["far"], 5, torch.float64)  # (b, v, D) depths
    assert ref.rel_l2(got, want.transpose(0, 1).reshape(v * b, 5)) < 1e-6
    assert torch.equal(depth_candidates(case["near"], case["far"], 1), (1.0 / case["far"]).t().reshape(-1, 1))
    with pytest.raises(ValueError):
        depth_candidates(case["near"], case["far"], 0)


def test_symbols_are_declared_exported_and_listed():
    import pf3plat_amd
    from pf3plat_amd import cost_volume

    assert pf3plat_amd.plane_sweep_cost_volume is cost_volume.plane_sweep_cost_volume and pf3plat_amd.depth_candidates is cost_volume.depth_candidates
    lib = _lib.load()
    assert lib.gsr_abi_version() == 5 == _lib.GSR_ABI_VERSION
    exported = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    assert "#define GSR_ABI_VERSION 5" in header
    for name in ("gsr_cost_volume", "gsr_cost_volume_backward", "gsr_cost_volume_scratch_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(exported, name) and f"{name}(" in header, name
    assert lib.gsr_cost_volume.restype is ctypes.c_int and len(lib.gsr_cost_volume.argtypes) == 14
    assert lib.gsr_cost_volume_backward.restype is ctypes.c_int and len(lib.gsr_cost_volume_backward.argtypes) == 15


def test_scratch_size_is_host_arithmetic():
    lib = _lib.load()
    size = lib.gsr_cost_volume_scratch_bytes
    assert size(2, 2, 8, 6, 9, 0) == 2 * 2 * 6 * 9 * 8 * 4 and size(2, 2, 8, 6, 9, 1) == 2 * size(2, 2, 8, 6, 9, 0)
    assert size(1, 3, 5, 7, 4, 0) == 3 * 7 * 4 * 8 * 4 and size(1, 2, 130, 8, 8, 1) == 2 * 2 * 64 * 132 * 4  # channels padded to 4
    assert size(14, 2, 256, 64, 64, 1) == 2 * 14 * 2 * 256 * 64 * 64 * 4
    assert size(0, 2, 8, 6, 9, 1) == 0
    for bad in ((-1, 2, 8, 6, 9), (1, 1, 8, 6, 9), (1, 2, 0, 6, 9), (1, 2, 8, 1, 9), (1, 2, 8, 6, 1), (1, 2, 256, 2048, 2048), (2 ** 15, 2 ** 15, 1, 2, 2)):
        assert size(*bad, 0) == 0 and size(*bad, 1) == 0, bad


def test_entry_points_refuse_invalid_arguments():
    """Every call below returns before a launch: nothing is read through the dummy pointer."""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = (2, 2, 8, 6, 9, 5)
    fwd = lambda sizes, ptrs: lib.gsr_cost_volume(*sizes, *ptrs, None)
    bwd = lambda sizes, ptrs: lib.gsr_cost_volume_backward(*sizes, *ptrs, None)
    for bad in ((-1, 2, 8, 6, 9, 5), (2, 1, 8, 6, 9, 5), (2, 0, 8, 6, 9, 5), (2, 2, 0, 6, 9, 5), (2, 2, 8, 1, 9, 5), (2, 2, 8, 6, 1, 5), (2, 2, 8, 6, 9, 0),
                (2, 2, 8, 6, 9, -3), (1, 2, 256, 2048, 2048, 1), (1, 2, 1, 1024, 1024, 1025), (2 ** 15, 2 ** 15, 1, 2, 2, 1)):
        assert fwd(bad, [p] * 7) == INVALID and bwd(bad, [p] * 8) == INVALID, bad
    for k in range(7):  # features, intrinsics, extrinsics, near, far, cost, scratch
        assert fwd(good, [None if q == k else p for q in range(7)]) == INVALID, k
    for k in range(8):  # ..., far, dL_dcost, dL_dfeatures, scratch
        assert bwd(good, [None if q == k else p for q in range(8)]) == INVALID, k
    assert fwd((0, 2, 8, 6, 9, 5), [p] * 7) == 0 and bwd((0, 2, 8, 6, 9, 5), [p] * 8) == 0  # no scene: nothing is launched


def test_python_checks_fire_in_order_and_refuse_cpu_tensors(monkeypatch):
    from pf3plat_amd import cost_volume as cv

    def no_load():
        raise AssertionError("the library was loaded before the checks were through")

    monkeypatch.setattr(_lib, "load", no_load)
    case = reference("v2")[0]
    f, k, e, n, fa = (case[x] for x in ("features", "intrinsics", "extrinsics", "near", "far"))
    bad = [((f[0], k, e, n, fa, 5), "features"), ((f[:, :1], k[:, :1], e[:, :1], n[:, :1], fa[:, :1], 5), "two views"),
           ((f[..., :1], k, e, n, fa, 5), "w >= 2"), ((f[..., :1, :], k, e, n, fa, 5), "h >= 2"), ((f, k[:, :, :2], e, n, fa, 5), "intrinsics"),
           ((f, k, e[:, :, :3], n, fa, 5), "extrinsics"), ((f, k, e, n[:1], fa, 5), "near, far"), ((f, k, e, n, fa[:, :1], 5), "near, far"),
           ((f, k, e, n, fa, 0), "depth candidate")]
    for args, word in bad:  # CPU tensors all of them: the shapes are judged first
        with pytest.raises(ValueError, match=word):
            cv.plane_sweep_cost_volume(*args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.plane_sweep_cost_volume(f, k, e, n, fa, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cv.plane_sweep_cost_volume(f.clone().requires_grad_(True), k, e, n, fa, 5)


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


def _hip(case, features=None, dtype=torch.float32, extr_grad=False, factor=1.0):
    """Forward + backward of the operator on the case: the volume, dL/dfeatures for factor x the case's cotangent, extrinsics.grad."""
    from pf3plat_amd.cost_volume import plane_sweep_cost_volume

    f = (case["features"].to(DEV, dtype) if features is None else features).detach().requires_grad_(True)
    e = case["extrinsics"].to(DEV, dtype).requires_grad_(extr_grad)
    cost = plane_sweep_cost_volume(f, case["intrinsics"].to(DEV, dtype), e, case["near"].to(DEV, dtype), case["far"].to(DEV, dtype), case["num"])
    assert cost.dtype == torch.float32 and cost.is_contiguous()
    (factor * cost).backward(case["cotangent"].to(DEV))
    assert f.grad.dtype == dtype and f.grad.shape == f.shape
    return cost.detach(), f.grad, e.grad


def _check_case(name, case, c64, g64, lv, lg):
    bv, bg = bars(lv, lg)
    cost, grad, e_grad = _hip(case, extr_grad=True)
    assert e_grad is None
    dv, dg = ref.rel_l2(cost, c64), ref.rel_l2(grad, g64)
    print(f"{name}: value {dv:.2e} (bar {bv:.2e}), gradient {dg:.2e} (bar {bg:.2e})")
    assert torch.isfinite(cost).all() and torch.isfinite(grad).all()
    assert dv <= bv and dg <= bg, (dv, bv, dg, bg)
    assert torch.equal((cost == 0).cpu(), c64 == 0)  # the samples that miss the image are exactly zero, and no others
    cost3, grad3, _ = _hip(case, factor=3.0)
    assert torch.equal(cost3, cost) and ref.rel_l2(grad3, 3 * g64) <= bg  # the value's bits repeat; the gradient's need not (atomics)
    cost_d, grad_d, _ = _hip(case, dtype=torch.float64)  # (the case's values are float32 numbers: the conversion is exact)
    assert torch.equal(cost_d, cost) and grad_d.dtype == torch.float64 and ref.rel_l2(grad_d, g64) <= bg
    padded = torch.zeros(*case["features"].shape[:-1], case["features"].shape[-1] + 3, device=DEV)
    padded[..., 1:-2] = case["features"].to(DEV)
    view = padded[..., 1:-2]
    assert not view.is_contiguous()
    cost_v, grad_v, _ = _hip(case, features=view)
    assert torch.equal(cost_v, cost) and ref.rel_l2(grad_v, g64) <= bg
    with torch.no_grad():
        from pf3plat_amd.cost_volume import plane_sweep_cost_volume

        plain = plane_sweep_cost_volume(*(case[x].to(DEV) for x in ("features", "intrinsics", "extrinsics", "near", "far")), case["num"])
    assert not plain.requires_grad and torch.equal(plain, cost)
    return cost, grad


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_matches_the_float64_restatement(name):
    _check_case(name, *reference(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["v2", "v3"])
def test_hip_on_the_reference_records(name):
    case, cost_ref, grad_ref = fixture_case(name)
    c64, g64, lv, lg = _yardstick(case)
    cost, grad = _check_case("fixture " + name, case, c64, g64, lv, lg)
    # against the reference's own float32 numbers: both sides within their bar of the float64 restatement
    bv, bg = bars(lv, lg)
    assert ref.rel_l2(cost, cost_ref) <= bv + 2e-5 and ref.rel_l2(grad, grad_ref) <= bg + 2e-5


@pytest.mark.gpu
def test_hip_behind_the_camera_is_exactly_zero():
    """The other camera turned by 180 degrees: every q_z is negative and clamped to 1e-3, px and py are of the order 1e3 .. 1e5 pixels."""
    case = ref.build_case(8, 2, 2, 8, 6, 9, 5, NEAR, kind="behind")
    c64, g64 = ref.value_and_grad(ref.cost_volume, case, torch.float64)
    assert float(c64.abs().max()) == 0 and float(g64.abs().max()) == 0  # the case is what it claims
    cost, grad, e_grad = _hip(case, extr_grad=True)
    assert e_grad is None
    assert torch.isfinite(cost).all() and torch.isfinite(grad).all()
    assert float(cost.abs().max()) == 0 and float(grad.abs().max()) == 0


def _at_end_of_allocation(t):
    """A copy of t on the device whose last element is the last element of its allocation."""
    n = t.numel()
    pad = (-n) % 128 or 128
    buf = torch.empty(n + pad, dtype=t.dtype, device=DEV)
    assert buf.untyped_storage().nbytes() == (n + pad) * t.element_size()
    view = buf[pad:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() + n * t.element_size() == buf.data_ptr() + buf.untyped_storage().nbytes()
    return view


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["plain", "end_of_allocation"])
def test_hip_identity_rig(placement):
    """Both views carry the same features, pose and K: every px is an integer up to float32 rounding, the right and lower taps weigh 0
    (or a rounding's worth), including the tap at x = w that lies outside for x = w - 1: cost[d] = |f|^2 / sqrt(c) for every d."""
    b, v, c, h, w, d = 1, 2, 8, 6, 9, 5
    case = ref.build_case(9, b, v, c, h, w, d, NEAR, kind="identity")
    c64, g64, lv, lg = _yardstick(case)
    f = case["features"].double()
    want = (f[:, 0] ** 2).sum(1) / c ** 0.5                                    # (b, h, w)
    assert ref.rel_l2(c64, want[:, None].expand(b, d, h, w).repeat(v, 1, 1, 1)) < 1e-6  # the case is what it claims
    bv, bg = bars(lv, lg)
    feats = _at_end_of_allocation(case["features"]) if placement == "end_of_allocation" else None
    cost, grad, _ = _hip(case, features=feats)
    dv, dg = ref.rel_l2(cost, c64), ref.rel_l2(grad, g64)
    print(f"identity ({placement}): value {dv:.2e} (bar {bv:.2e}), gradient {dg:.2e} (bar {bg:.2e})")
    assert torch.isfinite(cost).all() and torch.isfinite(grad).all()
    assert dv <= bv and dg <= bg


@pytest.mark.gpu
def test_hip_peak_memory_is_of_the_order_of_the_inputs():
    """(1, 2, 64, 32, 32, 128): the warped features alone would be 67 MB; forward + backward may raise the peak by 8 x (features + volume)."""
    from pf3plat_amd.cost_volume import plane_sweep_cost_volume

    b, v, c, h, w, d = 1, 2, 64, 32, 32, 128
    case = ref.build_case(10, b, v, c, h, w, d, NEAR)
    args = [case[x].to(DEV) for x in ("features", "intrinsics", "extrinsics", "near", "far")]
    cot = case["cotangent"].to(DEV)
    plane_sweep_cost_volume(*args, d)  # (the library and the device are up before anything is counted)
    f = args[0].clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    cost = plane_sweep_cost_volume(f, *args[1:], d)
    cost.backward(cot)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    allowed = 8 * 4 * (b * v * c * h * w + v * b * d * h * w)
    print(f"peak memory rises by {rise / 1e6:.2f} MB (allowed {allowed / 1e6:.2f} MB; the warped features would be {4 * v * b * c * d * h * w / 1e6:.1f} MB)")
    assert tuple(cost.shape) == (v * b, d, h, w) and f.grad is not None and torch.isfinite(f.grad).all()
    assert rise <= allowed, (rise, allowed)
    f2 = args[0].clone().requires_grad_(True)  # a forward that no backward follows allocates the volume and one copy of the features
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        cost2 = plane_sweep_cost_volume(f2, *args[1:], d)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before <= 4 * (b * v * c * h * w + v * b * d * h * w) + 4096
    assert torch.equal(cost2, cost.detach())
