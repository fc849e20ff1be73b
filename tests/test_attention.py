"""Multi-head attention and LightGlue's SelfBlock / CrossBlock on the device (pf3plat_amd.attention; definition: include/gsr.h)
against tests/attention_ref.py - the reference's lines restated, float64 the reference - and against the records of the reference's
own classes, tests/golden/attention_fixtures.npz and attention_fixtures_cross.npz.

Bars (docs/PARITY.md sections 18 and 20): per case and quantity the HIP result lies within max(FLOOR, 4 x |float32 restatement -
float64 restatement|) rel-L2 of the float64 restatement; FLOOR is the worst the float32 restatement loses over the cases; no bar is
above 1e-4.  Quantities that are zero in exact arithmetic are judged by a norm ratio."""
import ctypes
import functools
import math
import os

import pytest
import torch

from pf3plat_amd import _lib
from tests import attention_ref as ref

INVALID = -1
ALL = ref.KERNEL_RECORDS + tuple(ref.CASES)
QUANTITIES = ("out", "dq", "dk", "dv")


def norm(t):
    return float(t.double().norm())


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.KERNEL_RECORDS)
def test_restatement_reproduces_the_reference_records_at_kernel_level(name):
    rec = ref.kernel_records()[name]
    err = ref.rel_l2(ref.restatement(name)["out"], rec["context"])
    print(name, "context", err)
    assert err < 2e-5, (name, err)


@pytest.mark.parametrize("name", tuple(ref.RECORDS))
def test_restatement_reproduces_the_reference_records_at_module_level(name):
    rec, r64 = ref.record(name), ref.block_restatement(name)
    assert len(r64) >= 12
    for key, value in r64.items():
        err = ref.rel_l2(value, rec[key])
        print(name, key, err)
        assert value.shape == rec[key].shape and err < 2e-5, (name, key, err)
    _, kind, E, H, B, N, M, _, _ = ref.RECORDS[name]
    if kind == "self":
        assert tuple(rec["q"].shape) == (B, H, N, E // H) and tuple(rec["context"].shape) == (B, H, N, E // H)
    else:
        assert tuple(rec["qk0"].shape) == (B, H, N, E // H) and tuple(rec["v1"].shape) == (B, H, M, E // H) and tuple(rec["m1"].shape) == (B, H, M, E // H)
    assert {n: (s[1], s[2], s[3], s[4], s[5], s[6]) for n, s in ref.RECORDS.items()} == {
        "self_rot": ("self", 64, 2, 2, 70, 70), "self_plain": ("self", 24, 3, 2, 45, 45), "cross": ("cross", 64, 2, 2, 70, 150)}


@pytest.mark.parametrize("name", ALL)
def test_bars_stay_under_the_cap(name):
    """... and no case loses much more in float32 than the floors say (they are the worst loss on the machine they were measured on)."""
    bars = ref.bars(name)
    r64, r32 = ref.restatement(name), ref.restatement(name, torch.float32)
    for key, bar in bars.items():
        lost = ref.rel_l2(r32[key], r64[key])
        print(name, key, "float32 loses", lost, "bar", bar)
        assert bar <= ref.CAP and (name in ref.KERNEL_RECORDS or lost <= 2.0 * ref.FLOOR[key]), (name, key, lost, bar)


def test_floors_are_of_the_size_of_the_worst_float32_loss():
    for key, floor in ref.FLOOR.items():
        worst = max(ref.rel_l2(ref.restatement(n, torch.float32)[key], ref.restatement(n)[key]) for n in ref.CASES if key not in ref.ZERO_GRADS.get(n, ()))
        print(key, "worst float32 loss", worst, "floor", floor)
        # (the figure depends on the CPU's summation order - threads, vector width -: the order of magnitude is checked here, the
        # figures of the machine the floors were measured on are in docs/PARITY.md section 20)
        assert 0.5 * floor <= worst <= 2.0 * floor, (key, worst, floor)


def module_losses():
    return {(name, key): ref.rel_l2(ref.block_restatement(name, torch.float32)[key], value)
            for name in ref.RECORDS for key, value in ref.block_restatement(name).items()}


def test_module_floor_is_the_worst_float32_loss():
    losses = module_losses()
    worst = max(losses, key=losses.get)
    print("worst float32 loss of a block", worst, losses[worst], "floor", ref.MODULE_FLOOR)
    assert 0.5 * ref.MODULE_FLOOR <= losses[worst] <= 2.0 * ref.MODULE_FLOOR


def test_cases_meet_their_conditions():
    sizes = {name: c[1:6] for name, c in ref.CASES.items()}
    assert sizes == {"d32": (2, 4, 131, 131, 32), "cross": (2, 2, 70, 323, 32), "cross_wide": (1, 3, 323, 70, 8), "d1": (2, 2, 70, 45, 1),
                     "d5": (1, 3, 131, 200, 5), "d31": (1, 2, 100, 150, 31), "n1": (2, 2, 1, 77, 16), "m1": (2, 2, 40, 1, 16),
                     "ramp_up": (1, 2, 260, 517, 32), "ramp_down": (1, 2, 260, 517, 32), "peaked": (2, 2, 130, 260, 32), "select": (2, 3, 256, 256, 8)}
    assert ref.CASES["ramp_up"][6] == ref.CASES["ramp_down"][6] == 30.0 and ref.CASES["peaked"][6] == 40.0
    assert all(c[8] is None for n, c in ref.CASES.items() if n != "select") and ref.CASES["select"][8] == 0.5
    for name, c in ref.CASES.items():
        case = ref.case_of(name)
        B, H, N, M, D = c[1:6]
        assert tuple(case["q"].shape) == tuple(case["cotangent"].shape) == (B, H, N, D) and tuple(case["k"].shape) == tuple(case["v"].shape) == (B, H, M, D)
    s = ref.probabilities(ref.case_of("d32")["q"], ref.case_of("d32")["k"])[0]
    assert 3.5 < float(s.std()) < 4.5  # scores of standard deviation 4
    for name in ("ramp_up", "ramp_down", "peaked"):
        case = ref.case_of(name)
        s, p = ref.probabilities(case["q"], case["k"])
        M = s.shape[-1]
        assert float(p.max(-1).values.mean()) > 0.9, name
        where = float(s.argmax(-1).double().mean()) / M
        if name == "ramp_up":
            assert where > 0.8, where
        if name == "ramp_down":
            assert where < 0.2, where
        if name != "peaked":  # a kernel that exponentiates without the running maximum overflows
            assert torch.isinf(torch.exp(s.float())).any() and float(s.abs().max()) >= 200.0
    one, case = ref.restatement("m1", torch.float32), ref.case_of("m1")
    assert (one["out"] == case["v"].expand(-1, -1, 40, -1)).all() and not one["dq"].any() and not one["dk"].any()
    # select: scores 256 at j = pi(i) and at most 192 elsewhere; every other weight is at most 2^-92, and p v is v[pi(i)] exactly
    case, perm = ref.case_of("select"), ref.select_permutations(ref.CASES["select"][0], 2, 3, 256)
    assert len({tuple(perm[b, h].tolist()) for b in range(2) for h in range(3)}) == 6  # a permutation of its own per (batch, head)
    s, _ = ref.probabilities(case["q"], case["k"], 0.5)
    hot = torch.zeros_like(s).scatter_(3, perm[..., None], 1.0).bool()
    assert (s[hot] == 256.0).all() and float(s[~hot].max()) <= 192.0
    p32 = torch.softmax(s.float(), -1)
    assert (p32[hot] == 1.0).all() and float(p32[~hot].max()) <= 2.0 ** -92
    assert case["v"].abs().min() >= 1 and case["cotangent"].abs().min() >= 1 and case["v"].abs().max() <= 6 and (case["v"] == case["v"].round()).all()
    assert not torch.equal(case["v"][0, 0], case["v"][0, 1]) and not torch.equal(case["cotangent"][0, 0], case["cotangent"][0, 1])
    r32 = ref.restatement("select", torch.float32)
    gather = lambda t, idx: torch.gather(t, 2, idx[..., None].expand(-1, -1, -1, t.shape[-1]))
    assert torch.equal(r32["out"], gather(case["v"], perm))
    assert torch.equal(gather(r32["dv"], perm), case["cotangent"])
    for r in (ref.restatement("select"), r32):
        assert norm(r["dq"]) <= ref.ZERO_RATIO * norm(r["dv"]) and norm(r["dk"]) <= ref.ZERO_RATIO * norm(r["dv"])


def test_symbols_are_declared_exported_and_listed():
    import pf3plat_amd
    from pf3plat_amd import attention

    for name in ("multi_head_attention", "bidirectional_cross_attention", "apply_cached_rotary_emb", "LearnableFourierPositionalEncoding",
                 "SelfBlock", "CrossBlock"):
        assert getattr(pf3plat_amd, name) is getattr(attention, name)
    lib = _lib.load()
    assert lib.gsr_abi_version() == 5 == _lib.GSR_ABI_VERSION
    exported = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    for name in ("gsr_attention", "gsr_attention_backward", "gsr_attention_scratch_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(exported, name) and f"{name}(" in header, name
    assert len(lib.gsr_attention_scratch_bytes.argtypes) == 5 and len(lib.gsr_attention.argtypes) == 15
    assert len(lib.gsr_attention_backward.argtypes) == 20
    texts = []
    for name in ("gsr_attention.h", "gsr_mono_attention.h"):  # the operator's own header, and the mono kernels' that it builds on
        with open(os.path.join(os.path.dirname(_lib.SRC), name)) as f:
            texts.append(f.read())
    assert all(k in texts[0] for k in ("k_mha_fwd", "k_mha_bwd_kv", "k_mha_bwd_q", '#include "gsr_mono_attention.h"'))
    assert all(k in texts[1] for k in ("k_mono_attn_fwd", "k_mono_attn_bwd_kv", "k_mono_attn_bwd_q"))


def test_scratch_size_and_invalid_arguments_are_host_arithmetic():
    """Every call below returns before a launch: nothing is read through the pointers, which are NULL."""
    lib = _lib.load()
    size = lib.gsr_attention_scratch_bytes
    assert size(12, 4, 4097, 4097, 32) == 12 * 4 * 4097 * 4 and size(1, 1, 1, 1, 1) == 4 and size(2, 3, 100, 7, 32) == 2400
    assert size(8, 4, 4098, 8196, 32) == size(8, 4, 4098, 1, 32)  # B H N floats: the key count does not enter
    fwd = lambda sizes, scale=0.25: lib.gsr_attention(*sizes, scale, *([None] * 9))
    bwd = lambda sizes, scale=0.25: lib.gsr_attention_backward(*sizes, scale, *([None] * 14))
    bad = ((0, 4, 64, 64, 32), (-1, 4, 64, 64, 32), (1, 0, 64, 64, 32), (1, -2, 64, 64, 32), (1, 4, 0, 64, 32), (1, 4, -3, 64, 32),
           (1, 4, 64, 0, 32), (1, 4, 64, -1, 32), (1, 4, 64, 64, 0), (1, 4, 64, 64, 33), (1, 4, 64, 64, -1),
           (2 ** 16, 2 ** 15, 1, 1, 1), (1, 2, 1, 2 ** 25, 32), (1, 2, 2 ** 25, 1, 32), (2 ** 20, 2 ** 20, 2 ** 20, 1, 1))
    for sizes in bad:
        assert fwd(sizes) == INVALID and bwd(sizes) == INVALID and size(*sizes) == 0, sizes
    assert fwd((1, 4, 64, 64, 32)) == INVALID and bwd((1, 4, 64, 64, 32)) == INVALID  # good sizes, NULL required pointers
    for scale in (math.inf, -math.inf, math.nan):
        assert fwd((1, 4, 64, 64, 32), scale) == INVALID and bwd((1, 4, 64, 64, 32), scale) == INVALID
    # B H max(N, M) D <= 2^31 - 1, at its edge on either axis
    assert size(1, 2, 2 ** 25 - 1, 5, 32) == 4 * 2 * (2 ** 25 - 1) and size(1, 2, 2 ** 25, 5, 32) == 0
    assert size(1, 2, 5, 2 ** 25 - 1, 32) == 40 and size(1, 2, 5, 2 ** 25, 32) == 0
    assert size(1, 1, 2 ** 31 - 1, 1, 1) == 4 * (2 ** 31 - 1) and size(1, 1, 1, 2 ** 31 - 1, 2) == 0


def test_python_checks_fire_in_order_and_refuse_cpu_tensors(monkeypatch):
    from pf3plat_amd import attention as at

    def no_load():
        raise AssertionError("the library was loaded before the checks were through")

    monkeypatch.setattr(_lib, "load", no_load)
    q, k, v = torch.zeros(2, 3, 12, 8), torch.zeros(2, 3, 20, 8), torch.zeros(2, 3, 20, 8)
    bad = [((q[0], k, v), "expected q"), ((q, k[0], v), "expected k"), ((q, k[:1], v), "expected k"), ((q, k[:, :2], v), "expected k"),
           ((q, k[..., :4], v), "expected k"), ((q, k, v[:, :, :5]), "expected v"), ((q, k, v[..., :4]), "expected v"),
           ((torch.zeros(2, 3, 12, 33), torch.zeros(2, 3, 20, 33), torch.zeros(2, 3, 20, 33)), "D <= 32"),
           ((q[..., :0], k[..., :0], v[..., :0]), "D <= 32"), ((q[:0], k[:0], v[:0]), "N, M >= 1"), ((q, k[:, :, :0], v[:, :, :0]), "N, M >= 1")]
    for args, word in bad:  # CPU tensors all of them: the shapes are judged first
        with pytest.raises(ValueError, match=word):
            at.multi_head_attention(*args)
    with pytest.raises(ValueError, match="finite"):
        at.multi_head_attention(q, k, v, scale=float("inf"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        at.multi_head_attention(q, k, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        at.multi_head_attention(q.clone().requires_grad_(True), k, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        at.bidirectional_cross_attention(q, k, torch.zeros_like(q), v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        at.SelfBlock(24, 3)(torch.zeros(2, 12, 24))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        at.CrossBlock(24, 3)(torch.zeros(2, 12, 24), torch.zeros(2, 20, 24), need_x1=False)
    with pytest.raises(NotImplementedError):
        at.SelfBlock(24, 3)(torch.zeros(2, 12, 24), None, torch.ones(12, 12, dtype=torch.bool))
    with pytest.raises(NotImplementedError):
        at.CrossBlock(24, 3)(torch.zeros(2, 12, 24), torch.zeros(2, 20, 24), torch.ones(12, 20, dtype=torch.bool))


def test_blocks_load_the_reference_state_dicts_strictly():
    from pf3plat_amd import attention as at

    for name, (_, kind, E, H, *_rest) in ref.RECORDS.items():
        block = (at.SelfBlock if kind == "self" else at.CrossBlock)(E, H, False)
        state = ref.state_of(name)
        block.load_state_dict(state, strict=True)
        assert set(dict(block.named_parameters())) == set(state)
        assert torch.equal(block.ffn[3].weight, state["ffn.3.weight"])
    assert {"Wqkv.weight", "out_proj.bias", "ffn.0.weight", "ffn.1.bias", "ffn.3.weight"} <= set(ref.state_of("self_rot"))
    assert {"to_qk.weight", "to_v.bias", "to_out.weight", "ffn.0.weight", "ffn.1.bias", "ffn.3.weight"} <= set(ref.state_of("cross"))
    at.SelfBlock(128, 4, flash=True), at.CrossBlock(128, 4, flash=True)  # 32 channels per head; flash is accepted
    for cls in (at.SelfBlock, at.CrossBlock):
        with pytest.raises(ValueError):
            cls(132, 4)
    enc = at.LearnableFourierPositionalEncoding(2, 32, 32)(torch.zeros(2, 7, 2))
    assert tuple(enc.shape) == (2, 2, 1, 7, 32)
    t = torch.arange(8.0).reshape(1, 1, 1, 8)
    assert torch.equal(at.apply_cached_rotary_emb(torch.stack([torch.zeros_like(t), torch.ones_like(t)]), t), ref.rotate_half(t))


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


def mha(name):
    from pf3plat_amd import multi_head_attention

    scale = ref.scale_of(name) if name == "select" else None  # (None: the default, D ** -0.5)
    return lambda q, k, v: multi_head_attention(q, k, v, scale)


@functools.lru_cache(maxsize=None)
def hip(name):
    """The HIP result of a case, computed once and shared."""
    got = ref.evaluate(mha(name), ref.case_of(name), DEV)
    return {key: value.cpu() for key, value in got.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_hip_matches_the_float64_restatement(name):
    got, r64, bars = hip(name), ref.restatement(name), ref.bars(name)
    errs = {key: ref.rel_l2(got[key], r64[key]) for key in bars}
    print(name, {key: (errs[key], bars[key]) for key in bars})
    for key in QUANTITIES:
        assert got[key].shape == r64[key].shape and torch.isfinite(got[key]).all(), (name, key)
    for key in bars:
        assert errs[key] <= bars[key] <= ref.CAP, (name, key, errs[key], bars[key])
    for key in ref.ZERO_GRADS.get(name, ()):  # zero in exact arithmetic
        print(name, key, norm(got[key]), "against dv", norm(got["dv"]))
        assert norm(got[key]) <= ref.ZERO_RATIO * norm(got["dv"]), (name, key)
    if name in ref.KERNEL_RECORDS:  # ... and the reference's own context
        assert ref.rel_l2(got["out"], ref.kernel_records()[name]["context"]) <= 2 * bars["out"]


@pytest.mark.gpu
def test_hip_select_is_exact():
    """One-hot rows of small integers, a permutation per (batch, head): a swapped row / column store, a k order of P that is not V's or
    a head read at another head's offset shows in every element."""
    case, perm, got = ref.case_of("select"), ref.select_permutations(ref.CASES["select"][0], 2, 3, 256), hip("select")
    for b in range(2):
        for h in range(3):
            assert torch.equal(got["out"][b, h], case["v"][b, h][perm[b, h]]), (b, h)  # out[i] == v[pi(i)]
            assert torch.equal(got["dv"][b, h][perm[b, h]], case["cotangent"][b, h]), (b, h)  # dv[pi(i)] == dO[i]
    assert norm(got["dq"]) <= ref.ZERO_RATIO * norm(got["dv"]) and norm(got["dk"]) <= ref.ZERO_RATIO * norm(got["dv"])


@pytest.mark.gpu
def test_hip_one_key_gives_the_value_and_the_column_sum():
    case, got = ref.case_of("m1"), hip("m1")
    assert torch.equal(got["out"], case["v"].expand(-1, -1, 40, -1))
    column = case["cotangent"].double().sum(2, keepdim=True)
    err = ref.rel_l2(got["dv"], column)
    print("dv against the float64 column sum", err)
    assert err <= ref.FLOOR["dv"]
    assert norm(got["dq"]) <= ref.ZERO_RATIO * norm(got["dv"]) and norm(got["dk"]) <= ref.ZERO_RATIO * norm(got["dv"])


@pytest.mark.gpu
def test_hip_heads_and_batches_do_not_mix():
    from pf3plat_amd import multi_head_attention

    case, first = dict(ref.case_of("d32")), hip("d32")
    k = case["k"].clone()
    k[1, 2] = k[1, 2].flip(0) * 1.5
    case["k"] = k
    got = ref.evaluate(multi_head_attention, case, DEV)
    for key in QUANTITIES:
        value = got[key].cpu()
        for b in range(2):
            for h in range(4):
                same = torch.equal(value[b, h], first[key][b, h])
                assert same == ((b, h) != (1, 2)), (key, b, h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("d32", "d5"))
def test_hip_strided_operands_equal_their_contiguous_copies(name):
    """q, k, v as the reference's SelfBlock cuts them out of one (B, N, 3 H D) buffer, read where they lie."""
    from pf3plat_amd import attention as at

    case = ref.case_of(name)
    B, H, N, D = case["q"].shape
    M = case["k"].shape[2]
    n = min(N, M)
    parts = [case[key][:, :, :n] for key in ("q", "k", "v")]  # (B, H, n, D) each
    buf = torch.stack(parts, -1).permute(0, 2, 1, 3, 4).reshape(B, n, 3 * H * D).contiguous().to(DEV).requires_grad_(True)
    qkv = buf.unflatten(-1, (H, -1, 3)).transpose(1, 2)
    q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
    assert q.stride() == (3 * n * H * D, 3 * D, 3 * H * D, 3)
    for i, t in enumerate((q, k, v)):  # no copy: the pointer handed to the call is inside the buffer
        assert at._operand(t).data_ptr() == buf.data_ptr() + 4 * i and at._operand(t).stride() == t.stride()
    cot = case["cotangent"][:, :, :n].to(DEV)
    out = at.multi_head_attention(q, k, v)
    (dbuf,) = torch.autograd.grad(out, buf, cot)
    dparts = dbuf.reshape(B, n, H, D, 3).permute(0, 2, 1, 3, 4)
    plain = ref.evaluate(at.multi_head_attention, {"q": parts[0].contiguous(), "k": parts[1].contiguous(), "v": parts[2].contiguous(),
                                                   "cotangent": cot.cpu()}, DEV)
    assert torch.equal(out, plain["out"])
    for i, key in enumerate(("dq", "dk", "dv")):
        assert torch.equal(dparts[..., i], plain[key]), (name, key)
    # the reference's other layout: .unflatten(-1, (H, -1)).transpose(1, 2) of a (B, n, H D) array
    flat = parts[0].transpose(1, 2).reshape(B, n, H * D).contiguous().to(DEV)
    view = flat.unflatten(-1, (H, -1)).transpose(1, 2)
    assert view.stride() == (n * H * D, D, H * D, 1) and at._operand(view).data_ptr() == flat.data_ptr()
    assert torch.equal(at.multi_head_attention(view, k, v), plain["out"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("d32", "cross", "ramp_up"))
def test_hip_repeats_bit_for_bit(name):
    """Forward and every gradient: no atomics, every sum in a fixed order."""
    first = hip(name)
    again = ref.evaluate(mha(name), ref.case_of(name), DEV)
    for key in QUANTITIES:
        assert torch.equal(first[key], again[key].cpu()), (name, key)


@pytest.mark.gpu
def test_hip_gradient_subsets_dtypes_and_no_grad():
    from pf3plat_amd import multi_head_attention

    case, full = ref.case_of("cross_wide"), hip("cross_wide")
    q, k, v, cot = (case[key].to(DEV) for key in ("q", "k", "v", "cotangent"))
    for i, key in enumerate(("dq", "dk", "dv")):  # each gradient alone
        args = [t.clone().requires_grad_(i == j) for j, t in enumerate((q, k, v))]
        (grad,) = torch.autograd.grad(multi_head_attention(*args), args[i], cot)
        assert torch.equal(grad.cpu(), full[key]), key
    kd = k.double().requires_grad_(True)  # a float64 k: converted; its gradient comes back in float64
    out = multi_head_attention(q, kd, v.double())
    (dk,) = torch.autograd.grad(out, kd, cot.double())
    assert out.dtype == torch.float64 and dk.dtype == torch.float64
    assert torch.equal(out.float().cpu(), full["out"]) and torch.equal(dk.float().cpu(), full["dk"])
    with torch.no_grad():
        out = multi_head_attention(q, k, v)
    assert torch.equal(out.cpu(), full["out"]) and not out.requires_grad
    assert out.transpose(1, 2).is_contiguous()  # the transposed view of a (B, N, H, D) buffer


@pytest.mark.gpu
def test_hip_bidirectional_cross_attention():
    from pf3plat_amd import bidirectional_cross_attention, multi_head_attention

    case = ref.case_of("cross")
    g = torch.Generator().manual_seed(77)
    qk0, qk1, v1 = case["q"], case["k"], case["v"]
    v0 = torch.randn(qk0.shape, generator=g)
    scale = 32 ** -0.5
    r64, r32 = ref.bidirectional(qk0, qk1, v0, v1, scale), ref.bidirectional(qk0, qk1, v0, v1, scale, torch.float32)
    dev = [t.to(DEV) for t in (qk0, qk1, v0, v1)]
    m0, m1 = bidirectional_cross_attention(*dev)
    assert torch.equal(m0, multi_head_attention(dev[0], dev[1], dev[3])) and torch.equal(m1, multi_head_attention(dev[1], dev[0], dev[2]))
    for name, got, want, lost in (("m0", m0, r64[0], r32[0]), ("m1", m1, r64[1], r32[1])):
        bar = max(ref.FLOOR["out"], 4.0 * ref.rel_l2(lost, want))
        err = ref.rel_l2(got, want)
        print(name, err, "bar", bar)
        assert got.shape == want.shape and err <= bar <= ref.CAP, (name, err, bar)
    only, none = bidirectional_cross_attention(*dev, need_m1=False)
    assert none is None and torch.equal(only, m0)


def module_bars(name):
    r64, r32 = ref.block_restatement(name), ref.block_restatement(name, torch.float32)
    return {key: max(ref.MODULE_FLOOR, 4.0 * ref.rel_l2(r32[key], r64[key])) for key in r64}


def device_block(name):
    from pf3plat_amd import attention as at

    _, kind, E, H, *_ = ref.RECORDS[name]
    block = (at.SelfBlock if kind == "self" else at.CrossBlock)(E, H, False)
    block.load_state_dict(ref.state_of(name), strict=True)
    return block.to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("name", tuple(ref.RECORDS))
def test_hip_module_form_on_the_reference_records(name):
    """Outputs, input gradients, the encoding's gradient and every parameter gradient of the block."""
    got = ref.run_block(name, device=DEV, module=device_block(name))
    r64, rec, bars = ref.block_restatement(name), ref.record(name), module_bars(name)
    assert set(got) == set(r64) and ("denc" in got) == (name == "self_rot")
    for key, bar in bars.items():
        err, err_rec = ref.rel_l2(got[key], r64[key]), ref.rel_l2(got[key], rec[key])
        print(name, key, err, "bar", bar, "; against the record", err_rec)
        assert got[key].shape == r64[key].shape and torch.isfinite(got[key]).all()
        assert err <= bar <= ref.CAP and err_rec <= 2 * bar, (name, key, err, err_rec, bar)


@pytest.mark.gpu
def test_hip_cross_block_without_x1_keeps_the_bits_of_what_is_kept():
    """need_x1=False against the full block at a cotangent on x0' alone: x0', dx0, dx1 and every parameter gradient."""
    block, r = device_block("cross"), ref.record("cross")

    def run(need_x1):
        x0, x1 = r["x0"].to(DEV).requires_grad_(True), r["x1"].to(DEV).requires_grad_(True)
        o0, o1 = block(x0, x1, need_x1=need_x1)
        assert (o1 is None) == (not need_x1)
        params = dict(block.named_parameters())
        grads = torch.autograd.grad(o0, [x0, x1] + list(params.values()), r["cot0"].to(DEV))
        return {"out0": o0.detach(), "dx0": grads[0], "dx1": grads[1], **{n: g for n, g in zip(params, grads[2:])}}

    full, kept = run(True), run(False)
    for key in full:
        assert torch.equal(full[key], kept[key]), key


@pytest.mark.gpu
def test_hip_peak_memory_stays_below_one_score_array():
    from pf3plat_amd import multi_head_attention

    B, H, N, M, D = 1, 2, 1024, 2048, 32
    g = torch.Generator().manual_seed(5)
    q, k, v, cot = (torch.randn(B, H, n, D, generator=g).to(DEV).requires_grad_(True) for n in (N, M, M, N))
    multi_head_attention(q, k, v).backward(cot.detach())  # (the library is loaded, the allocator warm)
    q.grad = k.grad = v.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    multi_head_attention(q, k, v).backward(cot.detach())
    torch.cuda.synchronize()
    rose = torch.cuda.max_memory_allocated() - before
    print("peak rose by", rose, "bytes; one (B, H, N, M) float32 array:", B * H * N * M * 4)
    assert rose < B * H * N * M * 4 == 16 * 2 ** 20
    assert torch.isfinite(q.grad).all() and torch.isfinite(k.grad).all() and torch.isfinite(v.grad).all()
