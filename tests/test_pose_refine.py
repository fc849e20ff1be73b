"""The refined poses and the pose errors (pf3plat_amd.pose.refine_poses / pose_encoding / pose_errors; definition: include/gsr.h)
against tests/pose_refine_ref.py - the reference's lines restated, float64 the reference - and against
tests/golden/pose_refine_fixtures.npz, what the reference's own functions computed.

Bars (docs/PARITY.md section 19): per case and quantity the HIP result lies within max(FLOOR, 4 x |float32 restatement - float64
restatement|) of the float64 restatement, in the measures of pose_refine_ref.errors_between; FLOOR is the worst the float32
restatement loses over the cases and is never taken from the HIP result."""
import ctypes
import functools

import pytest
import torch

from pf3plat_amd import _lib
from tests import pose_refine_ref as ref

INVALID = -1
ALL = tuple(ref.RECORDS) + tuple(ref.CASES)
EPS32 = 2.0 ** -23


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.RECORDS)
def test_restatement_reproduces_the_reference_records(name):
    """float32: the same operations, so a few ulp of the array's largest entry at most (8: another host's torch takes its short sums
    and the LU in another order; on the host that made the records the difference is 0); float64: within what the
    recorded float32 arithmetic rounds - 64 ulp of the largest entry covers the LU of a 4 x 4 and the chains behind the gradients."""
    rec, r32, r64 = ref.record(name), ref.restatement(name, torch.float32), ref.restatement(name)
    assert tuple(rec["sync"].shape[:2]) == ref.RECORDS[name]
    assert torch.equal(ref.pose_encoding(rec["sync"]), rec["pose_enc"])
    for key in ref.POSE_KEYS:
        # (dgamma is ONE number, a sum of terms of both signs: its rounding has the scale of the terms' magnitudes, not of their sum)
        scale = r64["dgamma_scale"] if key == "dgamma" else float(rec[key].abs().max())
        d32, d64 = float((r32[key] - rec[key]).abs().max()), float((r64[key].float() - rec[key]).abs().max())
        print(name, key, "float32", d32 / (EPS32 * scale), "ulp; float64", d64 / (EPS32 * scale), "ulp")
        assert d32 <= 8 * EPS32 * scale and d64 <= 64 * EPS32 * scale, (name, key, d32, d64, scale)
    # the three logged scalars from the per-scene figures: .mean(), [0], and the per-scene distance ([0] at b = 1)
    for dtype, ulp in ((torch.float32, 8), (torch.float64, 64)):
        e = ref.restatement(name, dtype)
        for got, want in ((e["rotation"].mean(), rec["geodesic"]), (e["translation_angle"][0], rec["angle_degree"]),
                          (e["translation_distance"], rec["translation"])):
            assert float((got.float() - want).abs().max()) <= ulp * EPS32 * float(want.abs().max()), (name, dtype, got, want)


@pytest.mark.parametrize("name", ("record_b", "b2v3", "b4v3_skewed", "b4v3_gamma0", "b33v8"))
def test_rigid_inverse_has_the_gradients_of_torch_inverse(name):
    """float64: [R^T | -R^T t], the form the kernel takes, against autograd through `.inverse()`, every cotangent mode; view 0 gets
    exactly nothing."""
    case = ref.case_of(name)
    for mode in ref.MODES:
        lu = ref.restatement(name, torch.float64, mode)
        rigid = ref.evaluate(lambda s, d, g: ref.refine(s, d, g, torch.float64, rigid=True), case, mode, dtype=torch.float64)
        for key in ("c2w", "w2c", "ddelta", "dgamma"):
            assert float((rigid[key] - lu[key]).abs().max()) <= 1e-13 * max(1.0, float(lu[key].abs().max())), (name, mode, key)
        assert not rigid["ddelta"][:, 0].any() and not lu["dfull"][:, 0].any() and not lu["dfull"][..., 9:].any()
    assert float(lu["ddelta"].abs().max()) > 0 or case["gamma"] == 0.0


def test_floors_are_of_the_size_of_the_worst_float32_loss():
    worst = {}
    for name in ref.CASES:
        for mode in ref.MODES:
            for key, lost in ref.float32_loss(name, mode).items():
                worst[key] = max(worst.get(key, 0.0), lost)
    print({key: (worst[key], ref.FLOOR[key]) for key in ref.FLOOR})
    for key, floor in ref.FLOOR.items():
        assert 0.5 * floor <= worst[key] <= 2.0 * floor, (key, worst[key], floor)


def test_cases_meet_their_conditions():
    sizes = {name: ref.CASES[name][1:3] for name in ref.CASES}
    assert set(sizes.values()) == {(1, 1), (1, 2), (2, 3), (4, 3), (33, 8), (129, 2), (65, 8)}
    assert {c[4] for c in ref.CASES.values()} == {1.0, 0.0, -0.7} and {c[3] for c in ref.CASES.values()} == {"plain", "skewed", "eye0"}
    for name in ALL:
        case = ref.case_of(name)
        b, v = case["sync"].shape[:2]
        assert case["full"].shape == (b, v, ref.CHANNELS) and float(case["full"][..., 9:].abs().mean()) > 100.0  # nothing may read these
        assert float(case["full"][..., :9].abs().max()) < 0.5
        assert ref.min_sin(case["sync"], case["full"], case["gamma"]) >= ref.MIN_SIN, name
        if v >= 2:
            e = ref.restatement(name)
            for deg in (torch.rad2deg(e["rotation"]), e["translation_angle"]):
                assert ref.ANGLES[0] <= float(deg.min()) and float(deg.max()) <= ref.ANGLES[1], (name, deg)
    skew = ref.case_of("b4v3_skewed")["sync"].double()
    a1, a2 = skew[..., 0, :3], skew[..., 1, :3]
    assert torch.allclose(a1.norm(dim=-1), torch.full((4, 3), 3.0, dtype=torch.float64), atol=1e-6) and float((a1 * a2).sum(-1).abs().min()) > 2.0
    assert torch.equal(ref.case_of("b2v3_eye0")["sync"][:, 0], torch.eye(4).expand(2, 4, 4))


def test_symbols_are_declared_exported_and_listed():
    import pf3plat_amd
    from pf3plat_amd import pose

    for name in ("refine_poses", "pose_encoding", "pose_errors", "RefinedPoses", "PoseErrors"):
        assert getattr(pf3plat_amd, name) is getattr(pose, name)
    lib = _lib.load()
    assert lib.gsr_abi_version() == 5 == _lib.GSR_ABI_VERSION
    exported = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    for name in ("gsr_pose_refine", "gsr_pose_refine_backward", "gsr_pose_errors"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(exported, name) and f"{name}(" in header, name
    assert (len(lib.gsr_pose_refine.argtypes), len(lib.gsr_pose_refine_backward.argtypes), len(lib.gsr_pose_errors.argtypes)) == (9, 11, 6)


def test_invalid_arguments_are_host_arithmetic():
    """Every call below returns before a launch: nothing is read through the pointers, which are NULL or never followed."""
    lib = _lib.load()
    fwd = lambda b, v, stride: lib.gsr_pose_refine(b, v, None, None, stride, None, None, None, None)
    bwd = lambda b, v, stride: lib.gsr_pose_refine_backward(b, v, None, None, stride, None, None, None, None, None, None)
    err = lambda b, v: lib.gsr_pose_errors(b, v, None, None, None, None)
    for b, v, stride in ((1, 0, 9), (1, -1, 9), (-1, 2, 9), (2, 2, 8), (2, 2, 0), (2 ** 27, 1, 9), (2 ** 20, 8, 256), (2 ** 16, 2 ** 16, 9)):
        assert fwd(b, v, stride) == INVALID and bwd(b, v, stride) == INVALID, (b, v, stride)
    for b, v in ((1, 0), (-1, 2), (2 ** 27, 1), (2 ** 16, 2 ** 16)):
        assert err(b, v) == INVALID, (b, v)
    assert fwd(2, 3, 139) == INVALID and bwd(2, 3, 139) == INVALID and err(2, 3) == INVALID  # good sizes, NULL required pointers
    assert fwd(0, 3, 139) == 0 and bwd(0, 3, 139) == 0 and err(0, 3) == 0  # no scene: nothing is launched


def test_python_checks_fire_in_order_and_refuse_cpu_tensors(monkeypatch):
    from pf3plat_amd import pose

    def no_load():
        raise AssertionError("the library was loaded before the checks were through")

    monkeypatch.setattr(_lib, "load", no_load)
    sync, delta, ext = torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 9), torch.zeros(2, 3, 4, 4)
    bad = [((sync[0], delta, 1.0), "sync_abspose"), ((sync[..., :3, :], delta, 1.0), "sync_abspose"), ((sync[:, :0], delta[:, :0], 1.0), "one view"),
           ((sync, delta[0], 1.0), "delta"), ((sync, torch.zeros(2, 3, 139), 1.0), "delta"), ((sync, delta[..., :6], 1.0), "delta"),
           ((sync, delta[:1], 1.0), r"\(b, v\)"), ((sync, delta[:, :2], 1.0), r"\(b, v\)"), ((sync, delta, torch.zeros(2)), "gamma")]
    for args, word in bad:  # CPU tensors all of them: the shapes are judged first
        with pytest.raises(ValueError, match=word):
            pose.refine_poses(*args)
    for args in ((sync, delta, 1.0), (sync, delta.clone().requires_grad_(True), torch.tensor(0.5, requires_grad=True))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pose.refine_poses(*args)
    for args, word in (((sync[0], ext), "c2w_pred"), ((sync, ext[..., :3, :]), "extrinsics_gt"), ((sync, ext[:1]), r"\(b, v\)"),
                       ((sync, ext[:, :2]), r"\(b, v\)"), ((sync[:, :0], ext[:, :0]), "one view")):
        with pytest.raises(ValueError, match=word):
            pose.pose_errors(*args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose.pose_errors(sync, ext)
    enc = pose.pose_encoding(ref.case_of("b2v3")["sync"])  # plain indexing: runs anywhere
    assert torch.equal(enc, ref.pose_encoding(ref.case_of("b2v3")["sync"])) and enc.shape == (2, 3, 9)
    with pytest.raises(ValueError, match="pose_encoding"):
        pose.pose_encoding(torch.zeros(2, 3, 9))


def test_delta_is_read_in_place_when_its_rows_are_uniform():
    from pf3plat_amd.pose import _delta_rows

    full = torch.zeros(4, 3, 139)
    view = full[..., :9]
    rows, stride = _delta_rows(view)
    assert rows.data_ptr() == full.data_ptr() and stride == 139
    assert _delta_rows(torch.zeros(4, 3, 9))[1] == 9 and _delta_rows(full[:1, :, 9:18])[1] == 139 and _delta_rows(full[:, :1, :9])[1] == 3 * 139
    for other in (full.double()[..., :9], full.permute(1, 0, 2)[..., :9], full[:, :, ::2][..., :9], torch.zeros(4, 9, 3).permute(0, 2, 1),
                  torch.zeros(4, 5, 139)[:, ::2, :9][:, :3]):
        rows, stride = _delta_rows(other)
        assert stride == 9 and rows.is_contiguous() and rows.dtype == torch.float32 and rows.shape == other.shape, other.stride()
    rows, stride = _delta_rows(torch.zeros(4, 6, 139)[:, ::2, :9])  # every second row of a parent: still uniform
    assert stride == 278


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def hip(name, mode="both", strided=True):
    """The HIP result of a case, computed once and shared."""
    from pf3plat_amd import pose_errors, refine_poses

    case = ref.case_of(name)
    got = ref.evaluate(refine_poses, case, mode, DEV, strided)
    if case["sync"].shape[1] >= 2 and mode == "both":
        got.update(pose_errors(got["c2w"], case["extrinsics"].to(DEV))._asdict())
    return {key: value.cpu() for key, value in got.items()}


def check(name, mode, got):
    r64, bars = ref.restatement(name, torch.float64, mode), {key: bar for key, bar in ref.bars(name, mode).items() if key in got}
    errs = ref.errors_between(got, r64, bars)
    print(name, mode, {key: (errs[key], bars[key]) for key in bars})
    for key in bars:
        assert got[key].shape == r64[key].shape and torch.isfinite(got[key]).all(), (name, mode, key)
        assert errs[key] <= bars[key] <= 2e-6, (name, mode, key, errs[key], bars[key])
    return bars


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_hip_matches_the_float64_restatement(name):
    got = hip(name)
    bars = check(name, "both", got)
    b, v = got["c2w"].shape[:2]
    assert ("rotation" in bars) == (v >= 2) and ("dgamma" in bars) == (v >= 2)
    eye, bottom = torch.eye(4), torch.tensor([0.0, 0.0, 0.0, 1.0])
    assert torch.equal(got["c2w"][..., 3, :], bottom.expand(b, v, 4)) and torch.equal(got["w2c"][..., 3, :], bottom.expand(b, v, 4))
    # c2w w2c = I to the bars: (C + dC)(W + dW) - I = dC W + C dW to first order, so over all poses
    # |C W - I| <= bar(c2w) |C| max_p |W_p| + max_p |C_p| bar(w2c) |W|  (Frobenius norms; the bars are relative to |C| and |W|)
    C, W = got["c2w"].double(), got["w2c"].double()
    per_pose = lambda m: float(m.flatten(2).norm(dim=-1).max())
    bound = bars["c2w"] * float(C.norm()) * per_pose(W) + per_pose(C) * bars["w2c"] * float(W.norm())
    off = float((C @ W - eye.double()).norm())
    print(name, "c2w w2c - I", off, "bound", bound)
    assert off <= bound, (name, off, bound)
    assert not got["dfull"][:, 0].any() and not got["dfull"][..., 9:].any()  # view 0 and the channels nothing reads
    if v == 1:
        assert not got["dfull"].any() and float(got["dgamma"]) == 0.0
    if ref.case_of(name)["gamma"] == 0.0:
        assert not got["dfull"].any() and float(got["dgamma"]) != 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("c2w", "w2c"))
@pytest.mark.parametrize("name", ("record_b", "b2v3", "b4v3_skewed", "b65v8"))
def test_hip_one_cotangent_alone(name, mode):
    got = hip(name, mode)
    check(name, mode, got)
    assert not got["dfull"][:, 0].any() and float(got["ddelta"].abs().max()) > 0


@pytest.mark.gpu
def test_hip_identity_first_view_is_exact():
    got = hip("b2v3_eye0")
    assert torch.equal(got["c2w"][:, 0], torch.eye(4).expand(2, 4, 4)) and torch.equal(got["w2c"][:, 0], torch.eye(4).expand(2, 4, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("record_a", "b4v3", "b33v8"))
def test_hip_strided_delta_equals_its_contiguous_copy(name):
    a, b = hip(name), hip(name, "both", False)
    for key in ("c2w", "w2c", "ddelta", "dgamma"):
        assert torch.equal(a[key], b[key]), (name, key)


@pytest.mark.gpu
def test_hip_backward_repeats_bit_for_bit_at_520_poses():
    from pf3plat_amd import refine_poses

    first = hip("b65v8_skewed")
    again = ref.evaluate(refine_poses, ref.case_of("b65v8_skewed"), "both", DEV)
    for key in ("c2w", "w2c", "ddelta", "dgamma"):
        assert torch.equal(first[key], again[key].cpu()), key


@pytest.mark.gpu
def test_hip_zero_rotation_row_gives_the_clamp_form():
    """Forward only: a1 = 0 in one pose, a2 = 0 in another; x / max(|x|, 1e-12) is 0 there, not NaN."""
    from pf3plat_amd import refine_poses

    case = ref.case_of("b4v3")
    sync, full = case["sync"].clone(), case["full"].clone()
    sync[0, 0, 0, :3] = 0.0
    sync[1, 0, 1, :3] = 0.0
    sync[2, 1, 0, :3], full[2, 1, :3] = 0.0, 0.0
    with torch.no_grad():
        got = refine_poses(sync.to(DEV), full.to(DEV)[..., :9], 1.0)
        want = ref.refine(sync, full, 1.0, rigid=True)  # (`.inverse()` refuses the singular matrices)
    assert torch.isfinite(got.c2w).all() and torch.isfinite(got.w2c).all()
    assert not got.c2w[0, 0, 0, :3].any() and not got.c2w[0, 0, 2, :3].any() and not got.c2w[1, 0, 1, :3].any() and not got.c2w[2, 1, 0, :3].any()
    assert ref.rel_l2(got.c2w, want[0]) <= ref.FLOOR["c2w"]  # (w2c: the reference inverts a singular matrix there)


@pytest.mark.gpu
def test_hip_pose_errors_exact_case_and_the_logged_scalars():
    from pf3plat_amd import pose_errors

    eye = torch.eye(4, device=DEV).expand(3, 2, 4, 4).contiguous()
    pred = eye.clone()
    pred[:, 1, :3, 3] = torch.tensor([0.0, 0.0, 2.0], device=DEV)  # (along an axis: t / |t| . t / |t| is exactly 1)
    pred[:, 0, :3, 3] = torch.tensor([7.0, 7.0, 7.0], device=DEV)  # (not the last view: not read)
    gt = eye.clone()
    gt[:, 0] = pred[:, 1]  # E[-1] = I, E[0] = the prediction: gt_rel is the prediction
    e = pose_errors(pred, gt)
    assert all(t.shape == (3,) and not t.any() for t in e), e
    nan = pose_errors(eye, gt)  # a zero predicted translation: 0 / 0, as the reference's
    assert torch.isnan(nan.translation_angle).all() and torch.isfinite(nan.rotation).all() and torch.isfinite(nan.translation_distance).all()
    for name in ref.RECORDS:
        rec, got = ref.record(name), hip(name)
        for value, want, key in ((got["rotation"].mean(), rec["geodesic"], "rotation"), (got["translation_angle"][0], rec["angle_degree"], "translation_angle"),
                                 (got["translation_distance"], rec["translation"], "translation_distance")):
            assert ref.rel_l2(value, want) <= 2 * ref.bars(name)[key], (name, key, value, want)  # (both sides carry a float32 loss)


@pytest.mark.gpu
def test_hip_module_form_dtypes_and_partial_requests():
    """As the encoder calls it: delta a view of the head's (b, v, 139) output, gamma an nn.Parameter; then float64 inputs, a Python
    float for gamma, and one gradient alone."""
    from pf3plat_amd import pose_encoding, refine_poses

    name = "b4v3_skewed"
    case, full_ref = ref.case_of(name), hip(name)
    head = torch.nn.Linear(5, ref.CHANNELS).to(DEV)
    gamma = torch.nn.Parameter(torch.tensor(case["gamma"], device=DEV))
    x = torch.randn(4, 3, 5, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():  # a head whose output IS the case's array
        head.weight.zero_()
        head.bias.zero_()
    delta_full = head(x) + case["full"].to(DEV)
    delta_full.retain_grad()
    out = refine_poses(case["sync"].to(DEV), delta_full[..., :9], gamma)
    ((out.c2w * case["cot_c2w"].to(DEV)).sum() + (out.w2c * case["cot_w2c"].to(DEV)).sum()).backward()
    got = {"c2w": out.c2w.detach().cpu(), "w2c": out.w2c.detach().cpu(), "ddelta": delta_full.grad[..., :9].cpu(), "dgamma": gamma.grad.cpu()}
    check(name, "both", got)
    assert gamma.grad.shape == () and not delta_full.grad[..., 9:].any() and head.bias.grad is not None
    for key in got:
        assert torch.equal(got[key], full_ref[key]), key
    assert torch.equal(pose_encoding(case["sync"].to(DEV)).cpu(), ref.pose_encoding(case["sync"]))
    # float64 inputs are converted, results and gradients come back in float64; a float gamma gets no gradient
    d64 = case["full"][..., :9].double().to(DEV).requires_grad_(True)
    out = refine_poses(case["sync"].double().to(DEV), d64, case["gamma"])
    (g64,) = torch.autograd.grad((out.c2w * case["cot_c2w"].to(DEV)).sum() + (out.w2c * case["cot_w2c"].to(DEV)).sum(), d64)
    assert out.c2w.dtype == out.w2c.dtype == g64.dtype == torch.float64
    assert torch.equal(out.c2w.float().cpu(), full_ref["c2w"]) and torch.equal(g64.float().cpu(), full_ref["ddelta"])
    # gamma's gradient alone
    g = torch.tensor([case["gamma"]], device=DEV, requires_grad=True)
    out = refine_poses(case["sync"].to(DEV), case["full"].to(DEV)[..., :9], g)
    (dg,) = torch.autograd.grad((out.c2w * case["cot_c2w"].to(DEV)).sum() + (out.w2c * case["cot_w2c"].to(DEV)).sum(), g)
    assert dg.shape == (1,) and torch.equal(dg.cpu()[0], full_ref["dgamma"])


@pytest.mark.gpu
def test_hip_render_gradient_reaches_the_pose_head():
    """End to end at (2, 3), 16 x 16, 64 Gaussians, shipped entry points only: refine_poses(...).c2w goes to the decoder, which inverts
    it in its camera set-up and - with its opt-in pose gradient - returns dL/dc2w; that cotangent, chained with the restatement's
    Jacobian in float64, is what arrives at delta and gamma."""
    import pf3plat_amd
    from pf3plat_amd import refine_poses, synthetic
    from pf3plat_amd.types import Gaussians

    b, v, hw, n = 2, 3, (16, 16), 64
    scenes = [synthetic.make_scene(50 + s, n, hw, num_views=v, near=1.5) for s in range(b)]
    cat = lambda pick: torch.cat([pick(sc) for sc in scenes]).to(DEV)
    gs = Gaussians(cat(lambda sc: sc.gaussians.means), cat(lambda sc: sc.gaussians.covariances), cat(lambda sc: sc.gaussians.harmonics),
                   cat(lambda sc: sc.gaussians.opacities))
    sync = cat(lambda sc: sc.extrinsics)
    rnd = torch.Generator().manual_seed(9)
    full = 1e3 * torch.randn(b, v, ref.CHANNELS, generator=rnd)
    full[..., :9] = 0.05 * torch.randn(b, v, 9, generator=rnd)
    full_dev = full.to(DEV).requires_grad_(True)
    gamma = torch.nn.Parameter(torch.tensor(0.5, device=DEV))
    weight = torch.rand((b, v, 3, *hw), generator=rnd).to(DEV)
    poses = refine_poses(sync, full_dev[..., :9], gamma)
    poses.c2w.retain_grad()
    dec = pf3plat_amd.DecoderSplattingCUDA(dataset_cfg=pf3plat_amd.decoder.DatasetCfgLike((0.2, 0.1, 0.0)))
    out = dec.forward(gs, poses.c2w, cat(lambda sc: sc.intrinsics), cat(lambda sc: sc.near), cat(lambda sc: sc.far), hw, pose_gradients=True)
    (out.color * weight).sum().backward()
    d_full, d_gamma, d_c2w = full_dev.grad.cpu(), gamma.grad.cpu(), poses.c2w.grad.cpu()
    assert torch.isfinite(d_full).all() and torch.isfinite(d_gamma) and float(d_gamma) != 0.0
    assert float(d_full[:, 1:, :9].norm(dim=-1).min()) > 0 and not d_full[:, 0].any() and not d_full[..., 9:].any()
    case = {"sync": sync.cpu(), "full": full, "gamma": 0.5, "cot_c2w": d_c2w, "cot_w2c": None}
    chain = {dtype: ref.evaluate(lambda s, d, g: ref.refine(s, d, g, dtype), case, "c2w", dtype=dtype) for dtype in (torch.float64, torch.float32)}
    delta = full.double()[..., :9]
    probe = torch.zeros_like(delta).requires_grad_(True)
    (denc,) = torch.autograd.grad((ref.refine(sync.cpu(), delta * 0.5 + probe, 1.0)[0] * d_c2w.double()).sum(), probe)
    chain[torch.float64]["dgamma_scale"] = float((delta[:, 1:] * denc[:, 1:]).abs().sum())
    keys = ("ddelta", "dgamma")
    lost = ref.errors_between(chain[torch.float32], chain[torch.float64], keys)
    errs = ref.errors_between({"ddelta": d_full[..., :9], "dgamma": d_gamma}, chain[torch.float64], keys)
    print({key: (errs[key], lost[key], ref.FLOOR[key]) for key in keys})
    for key in keys:
        assert errs[key] <= max(ref.FLOOR[key], 4.0 * lost[key]), (key, errs[key], lost[key])
