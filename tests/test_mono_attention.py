"""The mono-guided attention of the depth predictor (pf3plat_amd.mono_attention; definition: include/gsr.h) against
tests/mono_attention_ref.py - the reference's five lines restated, float64 the reference - and against
tests/golden/mono_attention_fixtures.npz, what the reference's own module computed.

Bars (docs/PARITY.md section 18): per case and quantity the HIP result lies within max(FLOOR, 4 x |float32 restatement - float64
restatement|) rel-L2 of the float64 restatement; FLOOR is the worst the float32 restatement loses over the cases; no bar is above
1e-4.  Quantities that are zero in exact arithmetic are judged by a norm ratio."""
import ctypes
import functools
import os

import pytest
import torch

from pf3plat_amd import _lib
from tests import mono_attention_ref as ref

INVALID = -1
ALL = ref.RECORDS + tuple(ref.CASES)


def scores(case):
    return torch.einsum("nei,nej->nij", case["q"].double(), case["k"].double())


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.RECORDS)
def test_restatement_reproduces_the_reference_records(name):
    rec, r64 = ref.record(name), ref.restatement(name)
    for key in ("out", "dq", "dk", "dv"):
        err = ref.rel_l2(r64[key], rec[key])
        print(name, key, err)
        assert err < 2e-5, (name, key, err)
    n, E, L = rec["q"].shape
    assert (E, L, rec["v"].shape[1]) == {"record_a": (8, 96, 128), "record_b": (2, 192, 32)}[name]


@pytest.mark.parametrize("name", ALL)
def test_bars_stay_under_the_cap(name):
    """... and no case loses much more in float32 than the floors say (they are the worst loss on the machine they were measured on)."""
    bars = ref.bars(name)
    r64, r32 = ref.restatement(name), ref.restatement(name, torch.float32)
    for key, bar in bars.items():
        lost = ref.rel_l2(r32[key], r64[key])
        print(name, key, "float32 loses", lost, "bar", bar)
        assert bar <= ref.CAP and (name in ref.RECORDS or lost <= 2.0 * ref.FLOOR[key]), (name, key, lost, bar)


def test_floors_are_of_the_size_of_the_worst_float32_loss():
    for key, floor in ref.FLOOR.items():
        worst = max(ref.rel_l2(ref.restatement(n, torch.float32)[key], ref.restatement(n)[key]) for n in ref.CASES if key not in ref.ZERO_GRADS.get(n, ()))
        # (the figure depends on the CPU's summation order - threads, vector width -: the order of magnitude is checked here, the
        # figures of the machine the floors were measured on are in docs/PARITY.md section 18)
        assert 0.5 * floor <= worst <= 2.0 * floor, (key, worst, floor)


def test_cases_meet_their_conditions():
    sizes = {name: (c[1], c[2], c[3], c[4]) for name, c in ref.CASES.items()}
    assert sizes == {"e8": (2, 8, 96, 128), "tail": (1, 8, 323, 128), "e1": (2, 1, 70, 32), "e2_c32": (2, 2, 192, 32), "e5_c130": (1, 5, 131, 130),
                     "e16": (1, 16, 150, 128), "e32": (1, 32, 100, 40), "l1": (2, 8, 1, 16), "c1": (1, 8, 65, 1), "ramp_up": (1, 8, 517, 128),
                     "ramp_down": (1, 8, 517, 128), "peaked": (2, 8, 260, 64), "flat": (1, 8, 200, 64), "select": (2, 8, 256, 128)}
    assert ref.CASES["ramp_up"][5] == ref.CASES["ramp_down"][5] == 30.0 and ref.CASES["peaked"][5] == 40.0
    for name in ("ramp_up", "ramp_down", "peaked"):
        s = scores(ref.case_of(name))
        L = s.shape[-1]
        assert float(torch.softmax(s, -1).max(-1).values.mean()) > 0.9, name
        where = float(s.argmax(-1).double().mean()) / L
        if name == "ramp_up":
            assert where > 0.8, where
        if name == "ramp_down":
            assert where < 0.2, where
        if name != "peaked":  # a kernel that exponentiates without the running maximum overflows
            assert torch.isinf(torch.exp(s.float())).any() and float(s.abs().max()) >= 200.0
    flat = ref.case_of("flat")
    assert (flat["k"] == flat["k"][:, :, :1]).all()
    for r in (ref.restatement("flat"), ref.restatement("flat", torch.float32)):  # dq is zero in exact arithmetic; float32 keeps it small
        assert float(r["dq"].double().norm()) <= 1e-5 * float(r["dk"].double().norm())
    one = ref.restatement("l1")
    assert (one["out"] == ref.case_of("l1")["v"]).all() and not one["dq"].any() and not one["dk"].any()
    # select: scores 512 at j = pi(i) and at most 384 elsewhere; p is exactly one-hot in float32
    case, perm = ref.case_of("select"), ref.select_permutations(ref.CASES["select"][0], 2, 256)
    s = scores(case)
    hot = torch.zeros_like(s).scatter_(2, perm[:, :, None], 1.0).bool()
    assert (s[hot] == 512.0).all() and float(s[~hot].max()) <= 384.0
    p32 = torch.softmax(s.float(), -1)
    assert (p32 == hot.float()).all()
    assert (case["v"][0, 3, 5], case["v"][0, 5, 3]) == ((3 * 3 + 7 * 5) % 11 - 5, (3 * 5 + 7 * 3) % 11 - 5) and case["v"][0, 3, 5] != case["v"][0, 5, 3]
    r32 = ref.restatement("select", torch.float32)
    for b in range(2):
        assert (r32["out"][b] == case["v"][b][:, perm[b]]).all()
        assert (r32["dv"][b][:, perm[b]] == case["cotangent"][b]).all()


def test_symbols_are_declared_exported_and_listed():
    import pf3plat_amd
    from pf3plat_amd import mono_attention

    assert pf3plat_amd.mono_guided_attention is mono_attention.mono_guided_attention
    lib = _lib.load()
    assert lib.gsr_abi_version() == 5 == _lib.GSR_ABI_VERSION
    exported = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    for name in ("gsr_mono_attention", "gsr_mono_attention_backward", "gsr_mono_attention_scratch_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(exported, name) and f"{name}(" in header, name
    assert len(lib.gsr_mono_attention_scratch_bytes.argtypes) == 4 and len(lib.gsr_mono_attention.argtypes) == 10
    assert len(lib.gsr_mono_attention_backward.argtypes) == 15
    with open(os.path.join(os.path.dirname(_lib.SRC), "gsr_mono_attention.h")) as f:  # the operator's own header
        text = f.read()
    assert all(k in text for k in ("k_mono_attn_fwd", "k_mono_attn_bwd_kv", "k_mono_attn_bwd_q", "__builtin_amdgcn_mfma_f32_32x32x2f32"))


def test_scratch_size_and_invalid_arguments_are_host_arithmetic():
    """Every call below returns before a launch: nothing is read through the pointers, which are NULL."""
    lib = _lib.load()
    size = lib.gsr_mono_attention_scratch_bytes
    assert size(8, 8, 4096, 128) == 8 * 4096 * 4 and size(1, 1, 1, 1) == 4 and size(2, 32, 100, 256) == 800
    for n, E, L, C in ((8, 8, 4096, 128), (3, 32, 1000, 256)):  # O(n L (E + C)): far below one (n, L, L) matrix
        assert size(n, E, L, C) <= 4 * n * L * (E + C) and size(n, E, 2 * L, C) == 2 * size(n, E, L, C)
    fwd = lambda sizes: lib.gsr_mono_attention(*sizes, *([None] * 6))
    bwd = lambda sizes: lib.gsr_mono_attention_backward(*sizes, *([None] * 11))
    bad = ((0, 8, 64, 16), (-1, 8, 64, 16), (1, 0, 64, 16), (1, 33, 64, 16), (1, 8, 0, 16), (1, 8, -5, 16), (1, 8, 64, 0), (1, 8, 64, 257),
           (1, 8, 2 ** 24, 128), (2 ** 20, 32, 2 ** 6, 1), (2 ** 16, 8, 2 ** 15, 16))
    for sizes in bad:
        assert fwd(sizes) == INVALID and bwd(sizes) == INVALID and size(*sizes) == 0, sizes
    assert fwd((1, 8, 64, 16)) == INVALID and bwd((1, 8, 64, 16)) == INVALID  # good sizes, NULL required pointers
    assert size(1, 32, 2 ** 26 - 1, 32) == 4 * (2 ** 26 - 1) and size(1, 32, 2 ** 26, 32) == 0  # n max(E, C) L <= 2^31 - 1


def test_python_checks_fire_in_order_and_refuse_cpu_tensors(monkeypatch):
    from pf3plat_amd import mono_attention as ma

    def no_load():
        raise AssertionError("the library was loaded before the checks were through")

    monkeypatch.setattr(_lib, "load", no_load)
    q, k, v = torch.zeros(2, 12, 8), torch.zeros(2, 8, 12), torch.zeros(2, 16, 12)
    bad = [((q[0], k, v), "mono_q"), ((q, k[:, :4], v), "mono_k"), ((q, k.permute(0, 2, 1), v), "mono_k"), ((q, k, v[:1]), "multi_v"),
           ((q, k, v[:, :, :5]), "multi_v"), ((q, k, v[0]), "multi_v"), ((torch.zeros(2, 12, 33), torch.zeros(2, 33, 12), v), "E <= 32"),
           ((q, k, torch.zeros(2, 257, 12)), "C <= 256"), ((q, k, torch.zeros(2, 0, 12)), "C <= 256"), ((q[:0], k[:0], v[:0]), "n >= 1")]
    for args, word in bad:  # CPU tensors all of them: the shapes are judged first
        with pytest.raises(ValueError, match=word):
            ma.mono_guided_attention(*args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ma.mono_guided_attention(q, k, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ma.mono_guided_attention(q.clone().requires_grad_(True), k, v)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def hip(name, strided_q=True):
    """The HIP result of a case, computed once and shared."""
    from pf3plat_amd import mono_guided_attention

    got = ref.evaluate(mono_guided_attention, ref.case_of(name), DEV, strided_q)
    return {key: value.cpu() for key, value in got.items()}


def norm(t):
    return float(t.double().norm())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_hip_matches_the_float64_restatement(name):
    got, r64, bars = hip(name), ref.restatement(name), ref.bars(name)
    errs = {key: ref.rel_l2(got[key], r64[key]) for key in bars}
    print(name, {key: (errs[key], bars[key]) for key in bars})
    for key in bars:
        assert got[key].shape == r64[key].shape and torch.isfinite(got[key]).all()
        assert errs[key] <= bars[key] <= ref.CAP, (name, key, errs[key], bars[key])
    for key in ref.ZERO_GRADS.get(name, ()):  # zero in exact arithmetic
        other = "dk" if name == "flat" else "dv"
        print(name, key, norm(got[key]), "against", other, norm(got[other]))
        assert torch.isfinite(got[key]).all() and norm(got[key]) <= 1e-5 * norm(got[other]), (name, key)


@pytest.mark.gpu
def test_hip_select_is_exact():
    """One-hot rows of small integers: a swapped row / column store or a k order of P that is not V's shows in every element."""
    case, perm, got = ref.case_of("select"), ref.select_permutations(ref.CASES["select"][0], 2, 256), hip("select")
    for b in range(2):
        assert torch.equal(got["out"][b], case["v"][b][:, perm[b]])  # out[:, :, i] == v[:, :, pi(i)]
        assert torch.equal(got["dv"][b][:, perm[b]], case["cotangent"][b])  # dv[:, :, j] == dO[:, :, pi^-1(j)]
    assert norm(got["dq"]) <= 1e-5 * norm(got["dv"]) and norm(got["dk"]) <= 1e-5 * norm(got["dv"])


@pytest.mark.gpu
def test_hip_one_key_gives_the_value_and_no_score_gradient():
    case, got = ref.case_of("l1"), hip("l1")
    assert torch.equal(got["out"], case["v"]) and torch.equal(got["dv"], case["cotangent"])
    assert not got["dq"].any() and not got["dk"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("tail", "ramp_up", "e5_c130"))
def test_hip_repeats_bit_for_bit(name):
    """Forward and every gradient: no atomics, every sum in a fixed order."""
    from pf3plat_amd import mono_guided_attention

    first = hip(name)
    again = ref.evaluate(mono_guided_attention, ref.case_of(name), DEV)
    for key in ("out", "dq", "dk", "dv"):
        assert torch.equal(first[key], again[key].cpu()), (name, key)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("record_a", "tail"))
def test_hip_strided_q_equals_its_contiguous_copy(name):
    from pf3plat_amd import mono_attention as ma

    q = ref.case_of(name)["q"].to(DEV)
    view = q.permute(0, 2, 1)
    assert view.stride() == (q.shape[1] * q.shape[2], 1, q.shape[2]) and ma._channel_major_q(view).data_ptr() == q.data_ptr()  # read where it lies
    a, b = hip(name), hip(name, False)
    for key in ("out", "dq", "dk", "dv"):
        assert torch.equal(a[key], b[key]), (name, key)


@pytest.mark.gpu
def test_hip_dtypes_layouts_and_partial_gradients():
    from pf3plat_amd import mono_guided_attention

    case, full = ref.case_of("e2_c32"), hip("e2_c32")
    q, k, v = (case[key].to(DEV) for key in ("q", "k", "v"))
    cot = case["cotangent"].to(DEV)
    kd = k.double().requires_grad_(True)  # a float64 k, a non-contiguous v: converted; gradients in the inputs' dtypes
    vt = v.permute(0, 2, 1).contiguous().permute(0, 2, 1).requires_grad_(True)
    out = mono_guided_attention(q.permute(0, 2, 1), kd, vt)
    dk, dv = torch.autograd.grad(out, (kd, vt), cot)
    assert out.dtype == torch.float32 and dk.dtype == torch.float64 and dv.dtype == torch.float32 and not vt.is_contiguous()
    assert torch.equal(out.cpu(), full["out"]) and torch.equal(dk.float().cpu(), full["dk"]) and torch.equal(dv.cpu(), full["dv"])
    qg = q.clone().requires_grad_(True)  # dq alone: the dK / dV pass is not launched
    (dq,) = torch.autograd.grad(mono_guided_attention(qg.permute(0, 2, 1), k, v), qg, cot)
    assert torch.equal(dq.cpu(), full["dq"])
    with torch.no_grad():
        assert torch.equal(mono_guided_attention(q.permute(0, 2, 1), k, v).cpu(), full["out"])


@pytest.mark.gpu
def test_hip_peak_memory_stays_below_one_score_matrix():
    from pf3plat_amd import mono_guided_attention

    n, E, L, C = 1, 8, 2048, 128
    g = torch.Generator().manual_seed(5)
    q, k, v, cot = (torch.randn(n, r, L, generator=g).to(DEV).requires_grad_(True) for r in (E, E, C, C))
    mono_guided_attention(q.permute(0, 2, 1), k, v).backward(cot.detach())  # (the library is loaded, the allocator warm)
    q.grad = k.grad = v.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    mono_guided_attention(q.permute(0, 2, 1), k, v).backward(cot.detach())
    torch.cuda.synchronize()
    rose = torch.cuda.max_memory_allocated() - before
    print("peak rose by", rose, "bytes; one (n, L, L) float32 matrix:", n * L * L * 4)
    assert rose < n * L * L * 4 == 16 * 2 ** 20
    assert torch.isfinite(q.grad).all() and torch.isfinite(k.grad).all() and torch.isfinite(v.grad).all()


@pytest.mark.gpu
def test_hip_module_form_on_the_reference_record():
    """mono_guided_attention followed by the reference's .view against the five eager lines in float32 on the device."""
    from pf3plat_amd import mono_guided_attention

    rec = ref.record("record_a")
    b_v, D, h_down, w_down = 2, 128, 8, 12
    q4, k4, v4 = (rec[key].to(DEV).view(b_v, -1, 2, 3) if key != "v" else rec[key].to(DEV).view(b_v, D, h_down, w_down) for key in ("q", "k", "v"))
    mono_q = q4.view(b_v, -1, h_down * w_down).permute(0, 2, 1)
    mono_k = k4.view(b_v, -1, h_down * w_down)
    multi_v = v4.view(b_v, -1, h_down * w_down)
    mono_atten = torch.softmax(torch.bmm(mono_q, mono_k), dim=-1)
    eager = torch.bmm(multi_v, mono_atten.permute(0, 2, 1)).view(b_v, D, h_down, w_down)
    fused = mono_guided_attention(mono_q, mono_k, multi_v).view(b_v, D, h_down, w_down)
    bar, r64 = ref.bars("record_a")["out"], ref.restatement("record_a")["out"].view(b_v, D, h_down, w_down)
    print("fused", ref.rel_l2(fused, r64), "eager", ref.rel_l2(eager, r64), "fused against eager", ref.rel_l2(fused, eager), "bar", bar)
    assert ref.rel_l2(fused, r64) <= bar and ref.rel_l2(fused, eager) <= 2 * bar
    assert ref.rel_l2(fused, rec["out"].view(b_v, D, h_down, w_down)) <= 2 * bar
