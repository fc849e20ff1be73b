"""The depth lift and the Pluecker ray map (pf3plat_amd.lift; gsr_lift_depth / gsr_lift_depth_backward / gsr_plucker_rays; definition:
include/gsr.h).

Yardstick: the float64 restatement of tests/lift_ref.py, itself pinned to the reference's own `sample_image_grid`, `unproject` and
`get_world_rays` by the records of tests/golden/lift_fixtures.npz (make_lift_fixtures.py).  Bars (docs/PARITY.md section 17, the
convention of sections 13 and 15): for xyz, the ray map and every gradient the HIP result lies within max(FLOOR, 4 x |float32
restatement - float64 restatement|) rel-L2 of the float64 restatement; FLOOR is the worst the float32 restatement loses over all the
cases below, measured on the CPU and rounded up in the second digit (`full_k` sets xyz 8.12e-8, d_depth_raw 7.65e-8, d_shift
6.95e-8 and the ray map 9.41e-8, `strip` d_intrinsics 4.45e-7; the other cases lose 3.3e-8 .. 4.8e-8 and 9.5e-8 .. 4.3e-7); no bar is
above 1e-4.  `depth` is bit-equal to the float32 restatement, the gradients' exact zeros are where the float32 restatement's are.  The cue is one-hot everywhere and its channel the float64
restatement's on every decided pixel (gap between the two smallest |down - hyp| above 1e-3 of the hypothesis spacing); at most 1 % of
a case's pixels may be undecided."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from pf3plat_amd import _lib
from tests import lift_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "lift_fixtures.npz")
# name: (seed, (b, v, h, w, D), kind)
CASES = {
    "fixture_a": (21, (2, 2, 8, 12, 128), "plain"),
    "fixture_b": (22, (1, 3, 13, 18, 128), "plain"),   # not multiples of 4: quarter grid 3 x 4, fractional bilinear weights
    "d1": (1, (1, 2, 8, 8, 1), "plain"),               # every pixel in channel 0
    "d5": (2, (1, 2, 8, 8, 5), "plain"),
    "d130": (3, (1, 2, 8, 8, 130), "plain"),           # past two waves of candidates
    "wide": (4, (1, 2, 4, 260, 128), "plain"),         # quarter width 65: a second cue workgroup of ONE pixel (scalar stores)
    "tall": (5, (1, 1, 68, 8, 128), "plain"),          # quarter height 17; v = 1
    "strip": (6, (1, 3, 32, 256, 128), "plain"),       # a strip at the reference's width: eight full workgroups and cue workgroups per image
    "per_view": (7, (2, 2, 8, 12, 128), "per_view"),   # near[0, 0], far[0, 0] differ from every other view's
    "full_k": (8, (1, 2, 8, 12, 128), "full_k"),       # skew and a general third row
    # the kernels' own partition: 1024 full-resolution pixels (four per thread) and 64 quarter pixels per workgroup
    "edge_tail": (9, (1, 1, 25, 41, 128), "plain"),    # 1025 pixels: the second workgroup holds a single pixel (scalar path)
    "edge_vec": (10, (1, 1, 16, 68, 128), "plain"),    # 1088 pixels, float4 path: a last workgroup of 64; 68 quarter pixels: a last float4
}
FLOOR = {"xyz": 8.2e-8, "d_depth_raw": 7.7e-8, "d_shift": 7.0e-8, "d_intrinsics": 4.5e-7, "plucker": 9.5e-8}
CAP = 1e-4
UNDECIDED_SHARE = 0.01
INVALID = -1  # GSR_ERR_INVALID_ARGUMENT of include/gsr.h
INPUTS = ("depth_raw", "shift", "near", "far", "intrinsics")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case, what the float64 and the float32 restatement give for it (computed once, shared, never modified)."""
    seed, shape, kind = CASES[name]
    case = ref.build_case(seed, *shape, kind)
    return case, ref.evaluate(case, torch.float64), ref.evaluate(case, torch.float32)


def plucker_size(name):
    _, (b, v, h, w, _), _ = CASES[name]
    return (17, 19) if name == "strip" else (h // 4, w // 4)  # (323 pixels: a second workgroup of 67)


@functools.lru_cache(maxsize=None)
def plucker_reference(name):
    case = reference(name)[0]
    H, W = plucker_size(name)
    return tuple(ref.plucker(case["c2w"].to(dt), case["intrinsics"].to(dt), H, W) for dt in (torch.float64, torch.float32))


def bar(quantity, r32, r64):
    b = max(FLOOR[quantity], 4 * ref.rel_l2(r32, r64))
    assert b <= CAP, (quantity, b)
    return b


def fixture(name):
    with np.load(FIXTURES) as fx:
        rec = {k.split(".", 1)[1]: torch.from_numpy(fx[k].astype(np.int64) if k.endswith("channel") else fx[k]) for k in fx.files if k.startswith(name + ".")}
    rec["num"] = int(rec["num"])
    return rec


# ---- without a GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fixture_a", "fixture_b"])
def test_restatement_reproduces_the_reference_record(name):
    rec = fixture(name)
    case, r64, r32 = reference(name)
    for k in INPUTS + ("c2w", "g_depth", "g_xyz"):
        assert torch.equal(rec[k], case[k]), k  # the record is of the case the GPU tests run
    assert rec["num"] == case["num"] == 128
    assert torch.equal(r32["depth"], rec["depth"])  # one rounding: the same bits
    _, (b, v, h, w, D), _ = CASES[name]
    assert tuple(rec["xyz"].shape) == (b, v, 3, h, w) and tuple(rec["channel"].shape) == (v * b, h // 4, w // 4)
    for q in ("xyz", "d_depth_raw", "d_shift", "d_intrinsics"):
        d = ref.rel_l2(rec[q], r64[q])
        print(f"{name}: record vs float64 restatement: {q} {d:.2e}")
        assert d < 2e-6, (q, d)
    assert torch.equal(r64["channel"], rec["channel"]) and torch.equal(r32["channel"], rec["channel"])
    p64, _ = plucker_reference(name)
    assert rec["plucker"].shape == p64.shape and ref.rel_l2(rec["plucker"], p64) < 2e-6


@pytest.mark.parametrize("name", list(CASES))
def test_cases_exercise_what_they_claim(name):
    """Conditions on the float64 restatement: 15-40 % of the pixels sit on a bound; at D = 128 at least min(D, quarter pixels) / 4
    distinct channels are hit and none holds more than 25 % of the pixels; at most 1 % of the quarter pixels are undecided and the
    float32 restatement agrees on the decided ones.  What the float32 restatement loses - the source of the floors - is printed."""
    case, r64, r32 = reference(name)
    _, (b, v, h, w, D), kind = CASES[name]
    lo, hi = case["near"].double().reshape(-1, 1, 1, 1), case["far"].double().reshape(-1, 1, 1, 1)
    on_bound = float(((r64["depth"] == lo) | (r64["depth"] == hi)).double().mean())
    assert 0.15 <= on_bound <= 0.40, on_bound
    for q in ("d_depth_raw", "d_shift"):  # the masks show in the gradients as exact zeros, in both precisions at the same pixels
        assert 0.10 <= float((r64[q] == 0).double().mean()) <= 0.60 and torch.equal(r64[q] == 0, r32[q] == 0)
    channel, gap = r64["channel"], r64["gap"]
    assert tuple(channel.shape) == (v * b, h // 4, w // 4) and int(channel.min()) >= 0 and int(channel.max()) < D
    decided = gap > 1e-3
    assert float((~decided).double().mean()) <= UNDECIDED_SHARE
    assert torch.equal(r32["channel"][decided], channel[decided])
    hit = int(channel.unique().numel())
    share = float(torch.bincount(channel.flatten(), minlength=D).max()) / channel.numel()
    losses = {q: ref.rel_l2(r32[q], r64[q]) for q in ("xyz", "d_depth_raw", "d_shift", "d_intrinsics")}
    losses["plucker"] = ref.rel_l2(*reversed(plucker_reference(name)))
    print(f"{name}: on a bound {on_bound:.3f}, channels hit {hit}, largest share {share:.3f}, undecided {int((~decided).sum())}, float32 loses "
          + ", ".join(f"{q} {e:.2e}" for q, e in losses.items()))
    for q, e in losses.items():
        assert e <= FLOOR[q] and 4 * e <= CAP, (q, e)  # FLOOR is the worst of these
    if D == 128:
        assert hit >= min(D, channel.numel()) / 4 and share <= 0.25, (hit, share)
    if D == 1:
        assert hit == 1 and int(channel.max()) == 0
    if kind == "per_view":  # hypotheses of the views' OWN bounds would name other channels on most pixels of the other views
        own = []
        for s in range(b):
            for i in range(v):
                hyp = ref.hypotheses(case["near"][s:s + 1, i:i + 1].double(), case["far"][s:s + 1, i:i + 1].double(), D, torch.float64)
                one = r64["depth"].reshape(b, v, 1, h, w)[s, i][None]
                own.append(ref.cue_channels(one, case["near"][:1, :1].double(), case["far"][:1, :1].double(), D, hyp=hyp)[0][0])
        own = torch.stack(own).reshape(b, v, h // 4, w // 4).transpose(0, 1).reshape(v * b, h // 4, w // 4)
        assert torch.equal(own[0], channel[0]) and float((own[1:] != channel[1:]).double().mean()) > 0.5
        assert float(case["near"][0, 0]) == 0.5 and float(case["far"][0, 0]) == 2.0 and (case["near"].flatten()[1:] > 0.54).all()
    if kind == "full_k":
        K = case["intrinsics"]
        assert (K[..., 0, 1] != 0).all() and (K[..., 1, 0] != 0).all() and (K[..., 2, :2] != 0).all() and (K[..., 2, 2] != 1).all()


def test_symbols_are_declared_exported_and_listed():
    import pf3plat_amd
    from pf3plat_amd import lift

    assert pf3plat_amd.lift_depth is lift.lift_depth and pf3plat_amd.plucker_rays is lift.plucker_rays and pf3plat_amd.LiftedDepth is lift.LiftedDepth
    assert lift.LiftedDepth._fields == ("depth", "xyz", "mono_cue")
    lib = _lib.load()
    assert lib.gsr_abi_version() == 5 == _lib.GSR_ABI_VERSION
    exported = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    for name in ("gsr_lift_depth", "gsr_lift_depth_backward", "gsr_lift_scratch_bytes", "gsr_plucker_rays"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(exported, name) and f"{name}(" in header, name
    assert len(lib.gsr_lift_depth.argtypes) == 15 and len(lib.gsr_lift_depth_backward.argtypes) == 16 and len(lib.gsr_plucker_rays.argtypes) == 8
    with open(os.path.join(os.path.dirname(_lib.SRC), "gsr_lift.h")) as f:  # the operator's own header
        text = f.read()
    assert all(k in text for k in ("k_lift_fwd", "k_lift_bwd", "k_lift_intr_finish", "k_plucker_rays"))


def test_scratch_size_and_invalid_arguments_are_host_arithmetic():
    """Every call below returns before a launch: nothing is read through the dummy pointer."""
    lib = _lib.load()
    size = lib.gsr_lift_scratch_bytes
    assert size(4, 3, 256, 256) == 12 * 64 * 9 * 8 and size(1, 1, 25, 41) == 2 * 9 * 8 and size(1, 2, 4, 4) == 2 * 9 * 8 and size(0, 2, 8, 8) == 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd = lambda sizes, ptrs: lib.gsr_lift_depth(*sizes, *ptrs, None)
    bwd = lambda sizes, ptrs: lib.gsr_lift_depth_backward(*sizes[:4], *ptrs, None)
    ray = lambda sizes, ptrs: lib.gsr_plucker_rays(*sizes, *ptrs, None)
    good = (2, 2, 8, 12, 128)
    bad_sizes = ((-1, 2, 8, 12), (2, 0, 8, 12), (2, 2, 3, 12), (2, 2, 8, 3), (1, 1, 32768, 32768), (2 ** 15, 2 ** 15, 4, 4))  # whatever D is
    for bad in bad_sizes:
        assert fwd(bad + (128,), [p] * 5 + [None] + [p] * 3) == INVALID and bwd(bad, [p] * 11) == INVALID and size(*bad) == 0, bad
    for bad in ((2, 2, 8, 12, 0), (2, 2, 8, 12, -1), (1, 2, 16384, 16384, 128), (1, 1, 1024, 1024, 2 ** 16)):  # D, or a cue past 2^31 - 1
        assert fwd(bad, [p] * 5 + [None] + [p] * 3) == INVALID, bad
    for k in (0, 1, 2, 3, 4, 6, 7, 8):  # every pointer but `lin` is required
        assert fwd(good, [None if q == k else p for q in range(9)]) == INVALID, k
    for k in range(5):
        assert bwd(good, [None if q == k else p for q in range(11)]) == INVALID, k
    assert bwd(good, [p] * 10 + [None]) == INVALID  # an intrinsics gradient without scratch
    assert fwd((0, 2, 8, 12, 128), [p] * 9) == 0 and bwd((0, 2, 8, 12, 128), [p] * 11) == 0  # no scene: nothing is launched
    for bad in ((-1, 2, 4, 4), (1, 0, 4, 4), (1, 2, 0, 4), (1, 2, 4, 0), (1, 1, 32768, 32768), (2 ** 15, 2 ** 15, 2, 2)):
        assert ray(bad, [p] * 3) == INVALID, bad
    for k in range(3):
        assert ray((1, 2, 4, 4), [None if q == k else p for q in range(3)]) == INVALID, k
    assert ray((0, 2, 4, 4), [p] * 3) == 0


def test_python_checks_fire_in_order_and_refuse_cpu_tensors(monkeypatch):
    from pf3plat_amd import lift

    def no_load():
        raise AssertionError("the library was loaded before the checks were through")

    monkeypatch.setattr(_lib, "load", no_load)
    case = reference("fixture_a")[0]
    r, s, n, f, k = (case[x] for x in INPUTS)
    bad = [((r, s, n[0], f, k), "near"), ((r, s, n, f[:1], k), "near, far"), ((r[0], s, n, f, k), "depth_raw"), ((r[:3], s, n, f, k), "depth_raw"),
           ((r[..., :3], s[..., :3], n, f, k), "w >= 4"), ((r[..., :3, :], s[..., :3, :], n, f, k), "h >= 4"), ((r, s[..., :8], n, f, k), "shift"),
           ((r, s, n, f, k[..., :2]), "intrinsics"), ((r, s, n, f, k, 0), "depth candidate")]
    for args, word in bad:  # CPU tensors all of them: the shapes are judged first
        with pytest.raises(ValueError, match=word):
            lift.lift_depth(*args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lift.lift_depth(r, s, n, f, k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lift.lift_depth(r.clone().requires_grad_(True), s, n, f, k, 5)
    c = case["c2w"]
    for args, word in [((c[0], k, (2, 3)), "c2w"), ((c, k[:1], (2, 3)), "intrinsics"), ((c, k, (2,)), "shape"), ((c, k, (0, 3)), "shape")]:
        with pytest.raises(ValueError, match=word):
            lift.plucker_rays(*args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lift.plucker_rays(c, k, (2, 3))


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


def _hip(case, stream=None, intr_grad=True, dtype=torch.float32):
    """Forward + backward of the operator on the case, on the current or on the given stream."""
    from pf3plat_amd.lift import lift_depth

    def go():
        raw, shift = (case[k].to(DEV, dtype).requires_grad_(True) for k in ("depth_raw", "shift"))
        near, far = (case[k].to(DEV, dtype).requires_grad_(True) for k in ("near", "far"))
        K = case["intrinsics"].to(DEV, dtype).requires_grad_(intr_grad)
        g_depth, g_xyz = case["g_depth"].to(DEV), case["g_xyz"].to(DEV)
        out = lift_depth(raw, shift, near, far, K, case["num"])
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in out) and not out.mono_cue.requires_grad
        torch.autograd.backward([out.depth, out.xyz], [g_depth, g_xyz])
        assert near.grad is None and far.grad is None and (K.grad is not None) == intr_grad
        assert raw.grad.dtype == dtype and raw.grad.shape == raw.shape and shift.grad.shape == shift.shape
        return {"depth": out.depth.detach(), "xyz": out.xyz.detach(), "cue": out.mono_cue, "d_depth_raw": raw.grad, "d_shift": shift.grad,
                "d_intrinsics": K.grad}

    if stream is None:
        res = go()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            res = go()
        torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    return {k: None if t is None else t.cpu() for k, t in res.items()}


def _check_cue(name, cue, r64, D):
    rows, _, hq, wq = cue.shape
    assert tuple(cue.shape) == (rows, D, hq, wq) == (r64["channel"].shape[0], D, *r64["channel"].shape[1:])
    assert bool(((cue == 0) | (cue == 1)).all()) and bool((cue.sum(1) == 1).all())  # exactly one 1 and D - 1 zeros
    channel = cue.argmax(1)
    decided = r64["gap"] > 1e-3
    skipped = float((~decided).double().mean())
    print(f"{name}: cue undecided share {skipped:.4f}, disagreements on undecided pixels {int((channel != r64['channel'])[~decided].sum())}")
    assert skipped <= UNDECIDED_SHARE
    assert torch.equal(channel[decided], r64["channel"][decided])
    return channel


def _check(name, case, r64, r32, got):
    assert torch.equal(got["depth"], r32["depth"])  # bit-equal to the float32 torch form
    report = []
    for q in ("xyz", "d_depth_raw", "d_shift", "d_intrinsics"):
        err, b = ref.rel_l2(got[q], r64[q]), bar(q, r32[q], r64[q])
        report.append(f"{q} {err:.2e} (bar {b:.2e})")
        assert torch.isfinite(got[q]).all() and err <= b, (name, q, err, b)
    print(f"{name}: " + ", ".join(report))
    for q in ("d_depth_raw", "d_shift"):  # the clamps' masks: exact zeros, at the float32 form's pixels and nowhere else
        assert torch.equal(got[q] == 0, r32[q] == 0), q
    return _check_cue(name, got["cue"], r64, case["num"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_matches_the_float64_restatement(name):
    """On the default stream against the bars; once more on a side stream: the same bits."""
    case, r64, r32 = reference(name)
    got = _hip(case)
    _check(name, case, r64, r32, got)
    side = _hip(case, stream=torch.cuda.Stream(device=DEV))
    for k, t in got.items():
        assert torch.equal(side[k], t), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fixture_a", "fixture_b"])
def test_hip_on_the_reference_records(name):
    """Against the reference's own float32 numbers: both sides within their bar of the float64 restatement."""
    from pf3plat_amd.lift import plucker_rays

    rec = fixture(name)
    case, r64, r32 = reference(name)
    got = _hip(rec)
    assert torch.equal(got["depth"], rec["depth"])
    for q in ("xyz", "d_depth_raw", "d_shift", "d_intrinsics"):
        assert ref.rel_l2(got[q], rec[q]) <= bar(q, r32[q], r64[q]) + 2e-6, q
    decided = r64["gap"] > 1e-3
    assert torch.equal(got["cue"].argmax(1)[decided], rec["channel"][decided])
    rays = plucker_rays(rec["c2w"].to(DEV), rec["intrinsics"].to(DEV), rec["plucker"].shape[-2:]).cpu()
    p64, p32 = plucker_reference(name)
    assert ref.rel_l2(rays, rec["plucker"]) <= bar("plucker", p32, p64) + 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_plucker_rays(name):
    from pf3plat_amd.lift import plucker_rays

    case = reference(name)[0]
    H, W = plucker_size(name)
    p64, p32 = plucker_reference(name)
    c2w, K = case["c2w"].to(DEV).requires_grad_(True), case["intrinsics"].to(DEV).requires_grad_(True)
    rays = plucker_rays(c2w, K, (H, W))
    assert rays.dtype == torch.float32 and tuple(rays.shape) == (c2w.shape[0] * c2w.shape[1], 6, H, W) and not rays.requires_grad
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = plucker_rays(c2w.double(), K.double(), (H, W))  # (float32 numbers: the conversion back is exact)
    torch.cuda.synchronize()
    err, b = ref.rel_l2(rays, p64), bar("plucker", p32, p64)
    print(f"{name}: ray map {H} x {W}: {err:.2e} (bar {b:.2e})")
    assert torch.isfinite(rays).all() and err <= b and torch.equal(again, rays)
    norm = rays[:, :3].double().norm(dim=1)
    assert float((norm - 1).abs().max()) < 1e-6  # unit directions; the moment is orthogonal to them
    assert float((rays[:, :3].double() * rays[:, 3:].double()).sum(1).abs().max()) < 1e-6


@pytest.mark.gpu
def test_hip_intrinsics_gradient_repeats_bit_for_bit_and_is_optional():
    case = reference("strip")[0]  # eight workgroups per image feed the second stage
    one, two = _hip(case), _hip(case)
    assert torch.equal(one["d_intrinsics"], two["d_intrinsics"]) and float(one["d_intrinsics"].abs().min()) > 0
    plain = _hip(case, intr_grad=False)
    assert plain["d_intrinsics"] is None
    for q in ("depth", "xyz", "cue", "d_depth_raw", "d_shift"):
        assert torch.equal(plain[q], one[q]), q
    wide = _hip(case, dtype=torch.float64)  # (the case's values are float32 numbers: the conversion is exact)
    assert wide["d_shift"].dtype == torch.float64 and all(torch.equal(wide[q].float(), one[q]) for q in ("depth", "xyz", "d_depth_raw", "d_shift", "d_intrinsics"))


@pytest.mark.gpu
def test_hip_single_cotangents_and_no_grad():
    """Only depth or only xyz used downstream: the other cotangent is absent, not a tensor of zeros."""
    from pf3plat_amd.lift import lift_depth

    case, r64, r32 = reference("fixture_b")
    args = lambda: [case[k].to(DEV).requires_grad_(k in ("depth_raw", "shift")) for k in INPUTS]
    a = args()
    lift_depth(*a).depth.backward(case["g_depth"].to(DEV))
    m2 = (r32["d_shift"] != 0).float()
    assert torch.equal(a[1].grad.cpu(), case["g_depth"] * m2)  # d_shift = m2 g_depth: exact
    a = args()
    lift_depth(*a).xyz.backward(case["g_xyz"].to(DEV))
    full = _hip(case)
    assert ref.rel_l2(a[1].grad.cpu() + case["g_depth"] * m2, full["d_shift"]) < 1e-6
    with torch.no_grad():
        out = lift_depth(*args())
    assert not out.depth.requires_grad and torch.equal(out.xyz.cpu(), full["xyz"]) and torch.equal(out.mono_cue.cpu(), full["cue"])


@pytest.mark.gpu
def test_hip_candidate_positions_may_be_passed():
    """The entry point with `lin` = torch's float32 linspace in device memory writes the cue it writes with NULL."""
    from pf3plat_amd.lift import lift_depth
    from pf3plat_amd.rasterizer import _stream_ptr

    case = reference("d130")[0]
    _, (b, v, h, w, D), _ = CASES["d130"]
    arrays = [case[k].to(DEV) for k in INPUTS]
    want = lift_depth(*arrays, D)
    lin = torch.linspace(0.0, 1.0, D, dtype=torch.float32).to(DEV)
    depth, xyz, cue = torch.empty_like(want.depth), torch.empty_like(want.xyz), torch.empty_like(want.mono_cue)
    rc = _lib.load().gsr_lift_depth(b, v, h, w, D, *(t.data_ptr() for t in arrays), lin.data_ptr(), depth.data_ptr(), xyz.data_ptr(), cue.data_ptr(),
                                    _stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(cue, want.mono_cue) and torch.equal(depth, want.depth) and torch.equal(xyz, want.xyz)


@pytest.mark.gpu
def test_hip_planted_non_finite_inputs():
    """A few NaN and infinite pixels in depth_raw: the cue stays one-hot with every channel in range, depth and xyz are non-finite
    exactly at the planted NaN pixels (an infinity is clamped to a bound: finite).  A property of valid memory behaviour."""
    from pf3plat_amd.lift import lift_depth

    case = dict(reference("fixture_b")[0])
    _, (b, v, h, w, D), _ = CASES["fixture_b"]
    raw = case["depth_raw"].clone()
    nan_at = [(0, 0, 0, 0), (1, 0, 5, 6), (2, 0, 12, 17)]
    inf_at = [(0, 0, 3, 3), (1, 0, 9, 2)]
    for at in nan_at:
        raw[at] = float("nan")
    raw[inf_at[0]], raw[inf_at[1]] = float("inf"), float("-inf")
    out = lift_depth(raw.to(DEV), *(case[k].to(DEV) for k in INPUTS[1:]), D)
    torch.cuda.synchronize()
    cue, depth, xyz = out.mono_cue.cpu(), out.depth.cpu(), out.xyz.cpu()
    assert bool(((cue == 0) | (cue == 1)).all()) and bool((cue.sum(1) == 1).all())
    planted = torch.zeros_like(raw, dtype=torch.bool)
    for at in nan_at:
        planted[at] = True
    assert torch.equal(~torch.isfinite(depth), planted)
    assert torch.equal(~torch.isfinite(xyz), planted.reshape(b, v, 1, h, w).expand(b, v, 3, h, w))
    want = ref.refined_depth(raw, case["shift"], case["near"], case["far"])
    assert torch.equal(depth[~planted], want[~planted])  # the neighbours, the clamped infinities included, as torch has them
    shift = case["shift"].clone()  # ... and a NaN shift is kept as well
    shift[0, 0, 1, 1] = float("nan")
    depth2 = lift_depth(case["depth_raw"].to(DEV), shift.to(DEV), *(case[k].to(DEV) for k in INPUTS[2:]), D).depth.cpu()
    assert bool(torch.isnan(depth2[0, 0, 1, 1])) and int((~torch.isfinite(depth2)).sum()) == 1


def _planted_two_views(seed=31, h=32, w=32):
    """One scene, two views at 32 x 32: smooth depths, a rigid motion between the cameras, and for every pixel of view 1 whose point
    lands inside view 0 a match (the pixel it lands in, its own pixel, score in .5 .. 1)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)
    ys, xs = torch.meshgrid(torch.linspace(0, 1, h, dtype=torch.float64), torch.linspace(0, 1, w, dtype=torch.float64), indexing="ij")
    raw = torch.stack([1.2 + 0.4 * torch.sin(3 * xs + k) * torch.cos(2 * ys) + 0.02 * u(h, w) for k in range(2)])[:, None]  # (2, 1, h, w)
    raw[:, :, :4] = 0.3 + 0.1 * u(2, 1, 4, w)  # a band of pixels below `near`: clamped, no gradient through m1
    shift = 0.05 * torch.randn(2, 1, h, w, generator=g, dtype=torch.float64)
    K = torch.tensor([[1.0, 0, 0.5], [0, 1.1, 0.5], [0, 0, 1]], dtype=torch.float64).expand(1, 2, 3, 3).clone()
    K[0, 1, 0, 0] = 0.95
    near, far = torch.full((1, 2), 0.5, dtype=torch.float64), torch.full((1, 2), 2.0, dtype=torch.float64)
    case = {"depth_raw": raw, "shift": shift, "near": near, "far": far, "intrinsics": K}
    case = {k: t.to(torch.float32) for k, t in case.items()}
    R, t = ref.rotation(torch.tensor([0.03, -0.05, 0.02], dtype=torch.float64)), torch.tensor([0.08, -0.03, 0.02], dtype=torch.float64)
    depth, xyz = ref.lift(*(case[k].double() for k in INPUTS))
    X1 = xyz[0, 1].reshape(3, -1)                                    # view 1's points in its own camera
    q = K[0, 0] @ (R @ X1 + t[:, None])
    px, py = q[0] / q[2] * w, q[1] / q[2] * h                        # pixel units in view 0
    ix, iy = torch.floor(px).long(), torch.floor(py).long()
    inside = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h) & (q[2] > 0)
    ids_j = torch.arange(h * w)[inside]
    ids_i = (iy * w + ix)[inside]
    score = (0.5 + 0.5 * u(h * w))[inside].to(torch.float32)
    points_2d = torch.stack([px, py], -1)[inside].to(torch.float32)
    corr = {(0, 1): [(ids_i, ids_j, score)]}
    conf = {(0, 1): torch.tensor([0.8], dtype=torch.float32)}
    return case, corr, conf, points_2d


@pytest.mark.gpu
def test_hip_chain_lift_coarse_poses_pose_loss_backward():
    """lift_depth -> coarse_poses -> pose_loss -> backward on a planted two-view scene: depth_raw.grad and shift.grad against float64
    autograd through tests/lift_ref.py and tests/pose_loss_ref.py, the poses constants as in the reference (the float64 side takes
    the poses the device found).  The chain's floor is the larger of this file's and of the pose loss's own gradient floor
    (tests/test_pose_loss.py: 3.9e-6 for dL/dxyz, what the lift's backward is fed)."""
    from pf3plat_amd import losses, pose
    from pf3plat_amd.lift import lift_depth
    from tests import pose_loss_ref

    h = w = 32
    case, corr, conf, points_2d = _planted_two_views(h=h, w=w)
    assert corr[(0, 1)][0][0].numel() > 300
    w2d, w3d = 0.3, 1.7
    raw, shift = (case[k].to(DEV).requires_grad_(True) for k in ("depth_raw", "shift"))
    near, far, K = (case[k].to(DEV) for k in ("near", "far", "intrinsics"))
    out = lift_depth(raw, shift, near, far, K)
    packed = losses.pack_correspondences({p: [tuple(t.to(DEV) for t in l) for l in ls] for p, ls in corr.items()}, {p: c.to(DEV) for p, c in conf.items()})
    K_px = K * torch.tensor([w, h, 1.0], device=DEV).reshape(3, 1)
    coarse = pose.coarse_poses(out.xyz.detach(), K_px, packed, points_2d=points_2d.to(DEV), hypotheses=256)
    poses = coarse.absolute.detach()
    assert int(coarse.status[0]) == 0 and int(coarse.inliers[0]) > 0.9 * packed.offsets[-1]  # the planted motion was found
    loss, _, _ = losses.pose_loss(out.xyz, out.depth, poses, K, packed, w2d, w3d)
    loss.backward()
    torch.cuda.synchronize()
    got = {"d_depth_raw": raw.grad.cpu(), "d_shift": shift.grad.cpu()}

    def restated(dtype):
        r, s = (case[k].to(dtype).requires_grad_(True) for k in ("depth_raw", "shift"))
        depth, xyz = ref.lift(r, s, case["near"].to(dtype), case["far"].to(dtype), case["intrinsics"].to(dtype))
        value = pose_loss_ref.pose_loss(xyz, depth, poses.cpu().to(dtype), case["intrinsics"].to(dtype), corr, conf, w2d, w3d, dtype=dtype)[0]
        value.backward()
        return float(value.detach()), {"d_depth_raw": r.grad, "d_shift": s.grad}

    v64, g64 = restated(torch.float64)
    v32, g32 = restated(torch.float32)
    assert abs(float(loss.detach()) - v64) <= max(2.3e-6, 4 * abs(v32 - v64) / abs(v64)) * abs(v64)
    for q in ("d_depth_raw", "d_shift"):
        err = ref.rel_l2(got[q], g64[q])
        b = max(FLOOR[q], 3.9e-6, 4 * ref.rel_l2(g32[q], g64[q]))
        print(f"chain: {q} {err:.2e} (bar {b:.2e}), float32 restatement loses {ref.rel_l2(g32[q], g64[q]):.2e}")
        assert b <= CAP and err <= b, (q, err, b)
        assert float(g64[q].abs().max()) > 0 and torch.equal(got[q][:, :, :4] == 0, g64[q][:, :, :4] == 0)
    assert float(got["d_depth_raw"][:, :, :4].abs().max()) == 0  # the band below `near`: m1 is false
