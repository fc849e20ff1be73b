"""The perceptual distance's head (gsr_lpips_head / _finish / _backward, pf3plat_amd.lpips, losses.LossLpips / compute_lpips) against
the definition in include/gsr.h restated in float64 (tests/lpips_ref.py; docs/PARITY.md section 23).

CPU: the float64 restatement's closed-form gradient is float64 autograd of the package's plain lines wherever no feature vector is
all zero, and is 0 exactly where autograd is NaN (the stated departure); every case contains what it claims; the bars stay under
the cap but for the two structural tensors lpips_ref names (the gradients of "near", which the GPU test holds to the cap itself); the state-dict loader; the step gate of LossLpips; CPU tensors raise.

GPU: values, per-layer values and every gradient tensor within max(FLOOR, 4 x |float32 restatement - float64 restatement|) rel-L2
of the float64 restatement on channel counts and pixel counts around the kernel's groups and runs, layer tables of one, two and
five rows, planted all-zero vectors (exact zeros), nearly equal and widely scaled features; nullable gradients; bits that repeat
and that do not depend on the batch; the module, the loss and the metric against the whole pipeline in float64 on the CPU.

Measured on one MI355X (docs/PARITY.md section 23; printed by `pytest -s tests/test_lpips.py -m gpu`): values 2.7e-9 to 8.0e-7, worst
ratio to a bar 0.18 ("p1x1"); gradients 6.9e-8 to 1.9e-7, worst ratio 0.16, and "near" 5.26e-5 against the cap of 1e-4 (0.53; its rule would allow 1.7e-4);
module value 2.9e-8, in0.grad 2.5e-6 against 9.5e-6 (0.27).  The finish pass past its first trips - 9 images, 65, 129 and 66 units an
image (section 23.1) -: values 2.3e-8 to 5.9e-8, gradients 1.1e-7 to 1.4e-7, worst ratio 0.12.
"""
import ctypes
import functools
import os
import types

import pytest
import torch

from pf3plat_amd import _lib
from tests import lpips_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sorted(ref.CASES)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def zero_vectors(t):
    return (t == 0).all(dim=1)  # (n, h, w)


@pytest.mark.parametrize("name", ALL)
def test_restatement_gradient_is_float64_autograd(name):
    """... of the package's plain lines; where a feature vector is all zero autograd is NaN on exactly that vector and the
    restatement is 0 there: the departure include/gsr.h states."""
    c = ref.make_case(name)
    fa = [t.double().requires_grad_() for t in c["fa"]]
    fb = [t.double().requires_grad_() for t in c["fb"]]
    value = ref.upstream_head(fa, fb, c["ws"])
    assert value.shape == (fa[0].shape[0], 1, 1, 1)
    (value[:, 0, 0, 0] * c["g"].double()).sum().backward()
    r64, _ = ref.reference(name)
    assert ref.rel_l2(value[:, 0, 0, 0].detach(), r64["values"]) <= 1e-14
    for leaves, mine, side in ((fa, r64["da"], "a"), (fb, r64["db"], "b")):
        for x, d, scale in zip(leaves, mine, ref.term_scale(name, side)):
            zero = zero_vectors(x.detach()).unsqueeze(1).expand_as(x)
            assert torch.equal(torch.isnan(x.grad), zero), name  # NaN exactly on the all-zero vectors
            assert (d[zero] == 0).all() and torch.isfinite(d).all()
            if not zero.all():  # (against the size of the gradient's terms: at C = 1 they cancel to ten digits)
                assert float((x.grad[~zero] - d[~zero]).abs().max()) <= 1e-13 * scale, name


def test_cases_meet_their_conditions():
    lib = _lib.load()
    slots = lib.gsr_lpips_head_channel_slots()
    run = lib.gsr_lpips_head_pixel_run
    assert slots == 64 and run(0) == 0 and run(1025) == 0
    # channel edges: one group below and at the slots, two groups one past them, the switches to 4, 8 and 16 groups
    chans = [ref.CASES[f"c{c}"][2][0][0] for c in (1, 5, 63, 64, 65, 192, 512, 1024)]
    assert chans == [1, 5, slots - 1, slots, slots + 1, 3 * slots, 8 * slots, 16 * slots]
    assert [256 // run(c) for c in chans] == [1, 1, 1, 1, 2, 4, 8, 16]
    assert all(ref.CASES[f"c{c}"][2][0][1:] == (7, 9) for c in chans)
    # pixel edges at C = 64: less than a run, one run exactly, one short of four runs, one pixel past two runs
    r = run(64)
    sizes = {n: ref.CASES[n][2][0][1] * ref.CASES[n][2][0][2] for n in ("p1x1", "p1x77", "p16x16", "p33x31", "run+1")}
    assert sizes["p1x1"] == 1 and sizes["p1x77"] < r and sizes["p16x16"] == r and sizes["p33x31"] == 4 * r - 1 and sizes["run+1"] == 2 * r + 1
    assert all(ref.CASES[n][2][0][0] == 64 for n in sizes)
    assert [(c, h) for c, h, _ in ref.CASES["pyramid"][2]] == [(64, 32), (128, 16), (256, 8), (512, 4), (512, 2)] and ref.CASES["pyramid"][1] == 3
    assert len(ref.CASES["one_layer"][2]) == 1 and len(ref.CASES["two_layers"][2]) == 2
    # the zero case: vectors planted in a only, b only and both, in every layer, and a whole all-zero image
    z = ref.make_case("zeros")
    for (za, zb, zab), a, b in zip(z["planted"], z["fa"], z["fb"]):
        assert int(za.sum()) > 0 and int(zb.sum()) > 0 and int(zab.sum()) > 0
        assert torch.equal(zero_vectors(a), za | zab) and torch.equal(zero_vectors(b), zb | zab)
        assert bool(zero_vectors(a)[1].all()) and not bool(zero_vectors(b)[1].all())
    # the near case: b / a - 1 of the size it claims, C = 512; the far case: ten decades
    n = ref.make_case("near")
    nz = n["fa"][0] != 0
    ratio = (n["fb"][0][nz].double() / n["fa"][0][nz].double() - 1).std()
    assert n["fa"][0].shape[1] == 512 and 0.9 * ref.NEAR <= float(ratio) <= 1.1 * ref.NEAR
    f = ref.make_case("far")["fa"][0]
    assert float(f.max()) >= 1e3 and float(f[f > 0].min()) <= 1e-6
    # about half zeros, of VGG-like magnitude
    p = ref.make_case("pyramid")["fa"][0]
    assert 0.45 <= float((p == 0).float().mean()) <= 0.55 and 1.0 <= float(p.max()) <= 20.0
    # every bar is under the cap, the structural tensors aside, whose losses are what lpips_ref says
    for name in ALL:
        for key, bar in ref.bars(name).items():
            if (name, key) in ref.STRUCTURAL:
                loss = ref.float32_losses(name)[key]
                assert bar > ref.CAP and 0.5 * ref.STRUCTURAL[(name, key)] <= loss <= 2.0 * ref.STRUCTURAL[(name, key)], (name, key, loss)
            else:
                assert bar <= ref.CAP, (name, key, bar)


def test_finish_cases_take_both_loops_of_the_finish_pass_past_their_first_trip():
    """lpips_finish (gsr_image.h) is one workgroup of four waves: wave v adds the images v, v + 4, ..., and a lane the units k, k + 64,
    ... of an image's layer.  "n9": three trips over the images for wave 0; "u65", "u129": two and three trips over the units;
    "u65c64": both.  What a later trip adds is more than a hundred bars of the values, and one image's value in another's place moves
    them by more than ten bars: a trip left out, or an image's sum stored for another, fails the GPU test."""
    run = _lib.load().gsr_lpips_head_pixel_run
    lanes, waves = 64, 4
    with open(os.path.join(ROOT, "pf3plat_amd", "csrc", "gsr_image.h")) as f:
        text = f.read()
    assert f"k < y.upi; k += {lanes})" in text and f"n < A.N; n += kLpThreads / {lanes})" in text and f"kLpThreads = {lanes * waves};" in text
    seen_images, seen_units = 0, 0
    for name, (images, units) in ref.FINISH_CASES.items():
        _, n, layers, kind = ref.CASES[name]
        c, (r64, _), bar = ref.make_case(name), ref.reference(name), ref.bars(name)["values"]
        assert kind == "relu" and n == images and tuple(-(-h * w // run(ch)) for ch, h, w in layers) == units
        seen_images, seen_units = max(seen_images, -(-n // waves)), max(seen_units, -(-max(units) // lanes))
        values = r64["values"]
        apart = ((values[:, None] - values[None, :]).abs() + values.norm() * torch.eye(n)).min() / values.norm()  # one image's value for another's
        print(f"{name}: the two nearest values of its {n} images are {float(apart):.3e} of the values apart; bar {bar:.3e}")
        assert float(apart) > 10.0 * bar, name
        for l, (ch, h, w) in enumerate(layers):  # per unit what the forward leaves for the finish, in float64
            a, b = c["fa"][l].double(), c["fb"][l].double()
            d = ((ref.normalise(a)[0] - ref.normalise(b)[0]) ** 2 * c["ws"][l].double().view(1, -1, 1, 1)).sum(1).reshape(n, h * w)
            pad = units[l] * run(ch) - h * w
            per_unit = torch.cat([d, d.new_zeros(n, pad)], 1).reshape(n, units[l], run(ch)).sum(2) / (h * w)
            assert ref.rel_l2(per_unit.sum(1), r64["per_layer"][:, l]) <= 1e-13
            for trip in range(1, -(-units[l] // lanes)):
                share = per_unit[:, trip * lanes:(trip + 1) * lanes].sum(1)
                print(f"{name}: layer {l}, {units[l]} units an image, trip {trip} adds {ref.rel_l2(values - share, values):.3e} of the values; bar {bar:.3e}")
                assert ref.rel_l2(values - share, values) > 100.0 * bar, (name, trip)
    assert seen_images >= 3 and seen_units >= 3  # three trips of either loop
    assert ref.FINISH_CASES["u65c64"][0] > waves and ref.FINISH_CASES["u65c64"][1][0] > lanes  # ... and two of both in one call
    assert set(ref.FINISH_CASES) <= set(ALL)


def test_floor_is_of_the_size_of_the_worst_float32_loss():
    worst = max(v for name in ALL for key, v in ref.float32_losses(name).items() if (name, key) not in ref.STRUCTURAL)
    print("worst float32 loss", worst, "FLOOR", ref.FLOOR)
    assert ref.FLOOR / 10 <= worst <= ref.FLOOR * 1.5 and 4 * ref.FLOOR <= ref.CAP


def test_symbols_are_declared_exported_and_listed():
    lib = _lib.load()
    exported = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    for name in ("gsr_lpips_head", "gsr_lpips_head_backward", "gsr_lpips_head_finish", "gsr_lpips_head_partials",
                 "gsr_lpips_head_pixel_run", "gsr_lpips_head_channel_slots"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(exported, name) and f"{name}(" in header, name
    assert lib.gsr_abi_version() == 5 and "GSR_LPIPS_MAX_LAYERS 5" in header
    assert ctypes.sizeof(_lib.GsrLpipsLayer) == 40 and ctypes.sizeof(_lib.GsrLpipsLayers) == 208
    assert len(lib.gsr_lpips_head.argtypes) == 4 and len(lib.gsr_lpips_head_finish.argtypes) == 6 and len(lib.gsr_lpips_head_backward.argtypes) == 6


def table(layers, ptr=8):
    t = _lib.GsrLpipsLayers()
    t.num_layers = len(layers)
    for l, (c, h, w) in enumerate(layers):
        t.layer[l].a, t.layer[l].b, t.layer[l].weight = ptr, ptr, ptr
        t.layer[l].channels, t.layer[l].height, t.layer[l].width = c, h, w
    return t


def test_partials_query_and_invalid_arguments_are_host_arithmetic():
    lib = _lib.load()
    run = lib.gsr_lpips_head_pixel_run
    q = lib.gsr_lpips_head_partials
    pyramid = [(64, 256, 256), (128, 128, 128), (256, 64, 64), (512, 32, 32), (512, 16, 16)]
    per_image = sum(-(-h * w // run(c)) for c, h, w in pyramid)
    assert q(12, table(pyramid)) == 12 * per_image and q(1, table(pyramid)) == per_image  # an image's units do not depend on the batch
    assert q(1, table([(64, 1, 1)])) == 1 and q(3, table([(1024, 1, 17)])) == 3 * 2
    for n, layers in ((0, pyramid), (-1, pyramid), (1, []), (1, pyramid + [(64, 1, 1)]), (1, [(0, 4, 4)]), (1, [(1025, 4, 4)]),
                      (1, [(64, 0, 4)]), (1, [(64, 4, 0)]), (1, [(64, 65536, 32768)]), (1 << 15, [(64, 1 << 15, 1 << 15)])):
        t = table(layers[:5])
        t.num_layers = len(layers)
        assert q(n, t) == 0, (n, layers)
        assert lib.gsr_lpips_head(n, t, 8, None) == -1 and lib.gsr_lpips_head_finish(n, t, 8, 8, 8, None) == -1
        assert lib.gsr_lpips_head_backward(n, t, 8, None, None, None) == -1
    ok = table([(64, 4, 4)])
    assert lib.gsr_lpips_head(1, ok, None, None) == -1 and lib.gsr_lpips_head(1, table([(64, 4, 4)], ptr=None), 8, None) == -1
    assert lib.gsr_lpips_head_finish(1, ok, None, 8, 8, None) == -1 and lib.gsr_lpips_head_finish(1, ok, 8, None, 8, None) == -1
    assert lib.gsr_lpips_head_finish(1, ok, 8, 8, None, None) == -1 and lib.gsr_lpips_head_backward(1, ok, None, None, None, None) == -1
    assert lib.gsr_lpips_head_backward(1, ok, 8, None, None, None) == 0  # nothing to write: nothing is launched
    # a launch takes at most 2^32 - 1 threads, 16 777 215 workgroups of 256: the query answers 0 from the first unit past that
    most = (1 << 24) - 1
    assert q(1, table([(1024, 1, run(1024) * most)])) == most and q(1, table([(1024, 1, run(1024) * most + 1)])) == 0
    assert q(most, table([(64, 1, 1)])) == most and q(most + 1, table([(64, 1, 1)])) == 0
    assert lib.gsr_lpips_head(most + 1, table([(64, 1, 1)]), 8, None) == -1


def upstream_state(module, aliases=True):
    state = {"scaling_layer.shift": module.shift.clone(), "scaling_layer.scale": module.scale.clone()}
    for k, s in enumerate(ref.VGG_SLICES):
        for i in s:
            state[f"net.slice{k + 1}.{i}.weight"] = torch.randn_like(getattr(module, f"conv{i}_weight"))
            state[f"net.slice{k + 1}.{i}.bias"] = torch.randn_like(getattr(module, f"conv{i}_bias"))
    for k, c in enumerate(ref.VGG_CHANNELS):
        state[f"lin{k}.model.1.weight"] = torch.rand(1, c, 1, 1)
        if aliases:
            state[f"lins.{k}.model.1.weight"] = state[f"lin{k}.model.1.weight"]
    return state


def test_state_dict_loader_is_strict_and_ignores_the_lins_aliases():
    from pf3plat_amd.lpips import LPIPS

    torch.manual_seed(0)
    m = LPIPS()
    assert not m.training and not m.train().training and not list(m.parameters()) and len(list(m.buffers())) == 2 + 26 + 5
    state = upstream_state(m)
    assert len(state) == 2 + 26 + 5 + 5
    m.load_lpips_state_dict(state)
    assert torch.equal(m.conv28_weight, state["net.slice5.28.weight"]) and torch.equal(m.lin3, state["lin3.model.1.weight"].reshape(-1))
    assert torch.equal(m.conv0_bias, state["net.slice1.0.bias"])
    again = LPIPS(state_dict=upstream_state(m, aliases=False))
    assert again.lin0.shape == (64,)
    for drop in ("net.slice3.12.bias", "lin4.model.1.weight", "scaling_layer.scale"):
        with pytest.raises(RuntimeError, match="missing"):
            m.load_lpips_state_dict({k: v for k, v in state.items() if k != drop})
    for extra in ("net.slice5.30.weight", "lin5.model.1.weight", "version"):
        with pytest.raises(RuntimeError, match="unexpected"):
            m.load_lpips_state_dict({**state, extra: torch.zeros(1)})
    with pytest.raises(RuntimeError, match="shape"):
        m.load_lpips_state_dict({**state, "lin0.model.1.weight": torch.zeros(1, 65, 1, 1)})
    assert not m.state_dict()  # non-persistent buffers, as the reference's convert_to_buffer(persistent=False): nothing in a checkpoint
    two = LPIPS(seed=1)
    assert torch.equal(LPIPS(seed=1).conv0_weight, two.conv0_weight) and not torch.equal(LPIPS(seed=2).conv0_weight, two.conv0_weight)
    assert float(two.lin0.min()) >= 0.0


def test_loss_before_its_step_is_zero_and_launches_nothing(monkeypatch):
    from pf3plat_amd import losses

    called = []
    monkeypatch.setattr(_lib, "load", lambda: called.append(1))
    loss = losses.LossLpips(losses.LossLpipsCfg(weight=0.05, apply_after_step=100), lpips=lambda *a, **k: called.append(2))
    pred = types.SimpleNamespace(color=torch.rand(1, 4, 3, 16, 16))
    batch = {"target": {"image": torch.rand(1, 4, 3, 16, 16)}}
    out = loss(pred, batch, None, 99)
    assert out.shape == () and out.dtype == torch.float32 and float(out) == 0.0 and not called


def test_cpu_tensors_raise():
    from pf3plat_amd import losses
    from pf3plat_amd.lpips import LPIPS, lpips_distance

    c = ref.make_case("one_layer")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lpips_distance(c["fa"], c["fb"], c["ws"])
    x = torch.rand(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LPIPS()(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.compute_lpips(x, x)
    loss = losses.LossLpips(losses.LossLpipsCfg(1.0, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss(types.SimpleNamespace(color=torch.rand(1, 4, 3, 16, 16)), {"target": {"image": torch.rand(1, 4, 3, 16, 16)}}, None, 0)
    with pytest.raises(ValueError):
        lpips_distance(c["fa"], c["fb"], [c["ws"][0][:-1]])
    with pytest.raises(ValueError):
        lpips_distance([], [], [])


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


def run_head(c, images=None, want_a=True, want_b=True):
    """The operator on a case (or on the images `images` of it) -> dict of host tensors; da / db None where not requested."""
    from pf3plat_amd.lpips import lpips_distance

    sl = slice(None) if images is None else images
    fa = [t[sl].contiguous().to(DEV).requires_grad_(want_a) for t in c["fa"]]
    fb = [t[sl].contiguous().to(DEV).requires_grad_(want_b) for t in c["fb"]]
    ws = [t.to(DEV) for t in c["ws"]]
    values, per_layer = lpips_distance(fa, fb, ws)
    assert values.shape == (fa[0].shape[0],) and per_layer.shape == (fa[0].shape[0], 5) and not per_layer.requires_grad
    assert values.requires_grad == (want_a or want_b)
    if want_a or want_b:
        (values * c["g"][sl].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return {"values": values.detach().cpu(), "per_layer": per_layer.cpu(),
            "da": [None if t.grad is None else t.grad.cpu() for t in fa], "db": [None if t.grad is None else t.grad.cpu() for t in fb]}


@functools.lru_cache(maxsize=None)
def hip(name):
    return run_head(ref.make_case(name))


def same_bits(x, y):
    return all(torch.equal(t, u) for (_, t), (_, u) in zip(ref.compared(x), ref.compared(y)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_hip_matches_the_float64_restatement(name):
    got, (r64, _), bars = hip(name), ref.reference(name), ref.bars(name)
    c = ref.make_case(name)
    for (key, mine), (_, want) in zip(ref.compared(got), ref.compared(r64)):
        err = ref.rel_l2(mine, want)
        print(f"{name:11s} {key:9s} err {err:.3e} bar {bars[key]:.3e} ratio {err / bars[key]:.3f}")
        assert mine.shape == want.shape and mine.dtype == torch.float32 and torch.isfinite(mine).all(), (name, key)
        assert err <= min(bars[key], ref.CAP), (name, key, err, bars[key])  # (no asserted bound is above the cap)
        assert bars[key] <= ref.CAP or (name, key) in ref.STRUCTURAL, (name, key)
    assert (got["per_layer"][:, len(c["fa"]):] == 0).all()
    for x, d in zip(c["fa"] + c["fb"], got["da"] + got["db"]):  # an all-zero vector's gradient is exactly 0
        zero = zero_vectors(x).unsqueeze(1).expand_as(x)
        assert (d[zero] == 0).all(), name


@pytest.mark.gpu
def test_hip_an_image_alone_has_the_bits_it_has_in_the_batch():
    c, whole = ref.make_case("pyramid"), hip("pyramid")
    for i in range(3):
        alone = run_head(c, images=slice(i, i + 1))
        assert torch.equal(alone["values"], whole["values"][i:i + 1]) and torch.equal(alone["per_layer"], whole["per_layer"][i:i + 1])
        for t, u in zip(alone["da"] + alone["db"], whole["da"] + whole["db"]):
            assert torch.equal(t, u[i:i + 1])


@pytest.mark.gpu
def test_hip_images_of_a_waves_later_trips_alone_have_the_bits_they_have_in_the_batch():
    """Images 4 and 8 of "n9" are wave 0's second and third: alone each is a wave's first."""
    c, whole = ref.make_case("n9"), hip("n9")
    for i in (4, 8):
        alone = run_head(c, images=slice(i, i + 1))
        assert torch.equal(alone["values"], whole["values"][i:i + 1]) and torch.equal(alone["per_layer"], whole["per_layer"][i:i + 1])
        for t, u in zip(alone["da"] + alone["db"], whole["da"] + whole["db"]):
            assert torch.equal(t, u[i:i + 1])


def assert_within_bars(name, key, mine):
    (r64, _), bar = ref.reference(name), ref.bars(name)[key]
    want = dict(ref.compared(r64))[key]
    err = ref.rel_l2(mine.cpu(), want)
    assert torch.isfinite(mine).all() and err <= bar <= ref.CAP, (name, key, err, bar)


@pytest.mark.gpu
@pytest.mark.parametrize("want_a,want_b", [(True, False), (False, True), (True, True), (False, False)])
def test_hip_nullable_gradients(want_a, want_b):
    """The side that is not asked for gets nothing (and costs nothing: its divisions are skipped, so the other side's bits may differ
    from the both-sides call's in the last place - each is held to the float64 restatement)."""
    c, both = ref.make_case("two_layers"), hip("two_layers")
    got = run_head(c, want_a=want_a, want_b=want_b)
    assert torch.equal(got["values"], both["values"]) and torch.equal(got["per_layer"], both["per_layer"])
    for side, mine, want in (("da", got["da"], want_a), ("db", got["db"], want_b)):
        for l, t in enumerate(mine):
            if want:
                assert_within_bars("two_layers", f"{side}{l}", t)
            else:
                assert t is None
    if want_a and want_b:
        assert same_bits(got, both)


@pytest.mark.gpu
def test_hip_mixed_requests_per_layer_write_only_what_is_asked():
    """dL/da of layer 0 and dL/db of layer 1 alone: the other two are neither computed nor stored."""
    from pf3plat_amd.lpips import lpips_distance

    c = ref.make_case("two_layers")
    fa = [t.to(DEV).requires_grad_(l == 0) for l, t in enumerate(c["fa"])]
    fb = [t.to(DEV).requires_grad_(l == 1) for l, t in enumerate(c["fb"])]
    values, _ = lpips_distance(fa, fb, [t.to(DEV) for t in c["ws"]])
    (values * c["g"].to(DEV)).sum().backward()
    assert fa[1].grad is None and fb[0].grad is None
    assert_within_bars("two_layers", "da0", fa[0].grad)
    assert_within_bars("two_layers", "db1", fb[1].grad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pyramid", "zeros", "c1024"])
def test_hip_repeats_bit_for_bit(name):
    assert same_bits(run_head(ref.make_case(name)), hip(name))


# ---- the module, the loss and the metric ----------------------------------------------------------------------------------------------
MODULE_SEED, IMAGE_SEED = 3, 11


@functools.lru_cache(maxsize=None)
def module_case():
    """Images (2, 3, 32, 32) in [0, 1), a cotangent, the module's buffers on the CPU, and the whole pipeline in float64 and float32 on
    the CPU with in0's gradient (normalize=False on images mapped to [-1, 1] by the caller)."""
    from pf3plat_amd.lpips import LPIPS

    gen = torch.Generator().manual_seed(IMAGE_SEED)
    x0, x1, g = torch.rand((2, 3, 32, 32), generator=gen), torch.rand((2, 3, 32, 32), generator=gen), 0.5 + torch.rand(2, generator=gen)
    module = LPIPS(seed=MODULE_SEED)
    buffers = {k: v.clone() for k, v in module.named_buffers()}
    out = {}
    for dtype in (torch.float64, torch.float32):
        leaf = (2 * x0 - 1).to(dtype).requires_grad_()
        value = ref.pipeline(buffers, leaf, 2 * x1 - 1, dtype)
        (value[:, 0, 0, 0] * g.to(dtype)).sum().backward()
        out[dtype] = (value.detach(), leaf.grad)
    return x0, x1, g, module, out


def module_value_bar():
    """max(FLOOR, 4 x the float32 pipeline's loss of the value): also what two float32 runs of the same pipeline may differ by (the
    device's convolutions do not promise the same bits twice; the head does, and test_hip_repeats_bit_for_bit holds it to that)."""
    out = module_case()[4]
    bar = max(ref.FLOOR, 4.0 * ref.rel_l2(out[torch.float32][0], out[torch.float64][0]))
    assert bar <= ref.CAP
    return bar


def memoised_features(module, monkeypatch):
    """`module.features` evaluated once per distinct input (compared by bits): the device's float32 convolutions do not promise the
    same bits twice, the head does - with the taps shared, two forms of one call are compared for EQUAL bits."""
    plain, seen = module.features, []

    def features(x):
        for key, taps in seen:
            if key.shape == x.shape and torch.equal(key, x):
                return taps
        seen.append((x.detach().clone(), plain(x)))
        return seen[-1][1]

    monkeypatch.setattr(module, "features", features)
    return seen


@pytest.mark.gpu
def test_hip_module_matches_the_pipeline_in_float64(monkeypatch):
    x0, x1, g, module, out = module_case()
    module = module.to(DEV)
    leaf = (2 * x0 - 1).to(DEV).requires_grad_()
    value = module(leaf, (2 * x1 - 1).to(DEV))
    assert value.shape == (2, 1, 1, 1)
    (value[:, 0, 0, 0] * g.to(DEV)).sum().backward()
    (v64, g64), (v32, g32) = out[torch.float64], out[torch.float32]
    for key, mine, want, f32 in (("value", value.detach().cpu(), v64, v32), ("in0.grad", leaf.grad.cpu(), g64, g32)):
        bar = max(ref.FLOOR, 4.0 * ref.rel_l2(f32, want))
        err = ref.rel_l2(mine, want)
        print(f"module {key:9s} err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
        assert torch.isfinite(mine).all() and err <= bar <= ref.CAP, (key, err, bar)
    # normalize=True is the caller's 2 x - 1: against float64 within the value's bar, and, on shared taps, bit for bit
    with torch.no_grad():
        assert ref.rel_l2(module(x0.to(DEV), x1.to(DEV), normalize=True).cpu(), v64) <= module_value_bar()
        seen = memoised_features(module, monkeypatch)
        assert torch.equal(module(x0.to(DEV), x1.to(DEV), normalize=True), module(2 * x0.to(DEV) - 1, 2 * x1.to(DEV) - 1))
        assert len(seen) == 2  # (two images, each through the convolutions once)


@pytest.mark.gpu
def test_hip_compute_lpips_is_the_module_without_a_gradient(monkeypatch):
    from pf3plat_amd import losses

    x0, x1, _, module, _ = module_case()
    module = module.to(DEV)
    memoised_features(module, monkeypatch)
    a, b = x0.to(DEV).requires_grad_(), x1.to(DEV)
    got = losses.compute_lpips(a, b, lpips=module)
    assert got.shape == (2,) and not got.requires_grad
    assert torch.equal(got, module(a, b, normalize=True)[:, 0, 0, 0].detach())
    # without a network: a module of its own per device, made on first use and kept; random weights unless it is given a state dict,
    # and making it without one warns
    losses._lpips_models.clear()
    with pytest.warns(UserWarning, match="RANDOM weights"):
        cached = losses.compute_lpips(a, b)
    assert cached.shape == (2,) and not cached.requires_grad and torch.isfinite(cached).all()
    assert losses._lpips_models[a.device] is not None and len(losses._lpips_models) == 1
    state = upstream_state(module, aliases=False)
    for k in [k for k in state if k.startswith(("net.", "lin"))]:  # the package's names, this module's weights
        i = k.split(".")
        state[k] = (getattr(module, f"conv{i[2]}_{i[3]}") if i[0] == "net" else getattr(module, i[0]).reshape(1, -1, 1, 1)).clone()
    import warnings

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        loaded = losses.compute_lpips(a, b, state_dict=state)
    assert not [w for w in caught if "RANDOM" in str(w.message)]
    assert ref.rel_l2(loaded, got) <= module_value_bar() and ref.rel_l2(cached, got) > 1e-3
    losses._lpips_models.clear()


@pytest.mark.gpu
def test_hip_loss_is_weight_times_the_mean_over_the_inner_views_and_reaches_the_prediction(monkeypatch):
    from pf3plat_amd import losses

    _, _, _, module, _ = module_case()
    module = module.to(DEV)
    memoised_features(module, monkeypatch)
    gen = torch.Generator().manual_seed(IMAGE_SEED + 1)
    color = torch.rand((2, 4, 3, 32, 32), generator=gen).to(DEV).requires_grad_()
    image = torch.rand((2, 4, 3, 32, 32), generator=gen).to(DEV)
    loss = losses.LossLpips(losses.LossLpipsCfg(weight=0.05, apply_after_step=10), lpips=module)
    value = loss(types.SimpleNamespace(color=color), {"target": {"image": image}}, None, 10)
    with torch.no_grad():  # (the same taps: equal bits)
        want = 0.05 * module(color[:, 1:-1].reshape(-1, 3, 32, 32), image[:, 1:-1].reshape(-1, 3, 32, 32), normalize=True).mean()
    assert value.shape == () and torch.equal(value.detach(), want)
    value.backward()
    grad = color.grad
    assert torch.isfinite(grad).all() and (grad[:, 0] == 0).all() and (grad[:, -1] == 0).all() and float(grad[:, 1:-1].abs().max()) > 0
    assert float(loss(types.SimpleNamespace(color=color), {"target": {"image": image}}, None, 9)) == 0.0
