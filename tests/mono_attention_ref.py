"""The yardstick of the mono-guided attention tests: the reference's five lines
(src/model/encoder/costvolume/depth_predictor_multiview.py:360-366) restated as a torch function with a dtype switch - float64 is the
reference, float32 measures what the reference's own arithmetic loses -, the seeded cases, and rel_l2.  CPU only."""
import functools
import math
import os

import numpy as np
import torch

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mono_attention_fixtures.npz")
RECORDS = ("record_a", "record_b")  # what the reference's own module computed: tests/golden/make_mono_attention_fixtures.py

CAP = 1e-4  # no bar of a test is above this
# What the float32 restatement loses against float64 at worst over CASES (rel-L2; measured on the CPU by
# tests/test_mono_attention.py::test_bars_stay_under_the_cap, which prints it; rounded up in the second digit): the floor of the bars of the GPU tests.
FLOOR = {"out": 2.6e-6, "dq": 8.6e-6, "dk": 8.1e-6, "dv": 2.5e-6}

# name: (seed, n, E, L, C, amp, pattern).  q and k are normal with variance amp / sqrt(E): the scores, sums of E products, have standard
# deviation amp unless the pattern says otherwise.
CASES = {
    "e8": (1, 2, 8, 96, 128, 4.0, "random"),
    "tail": (2, 1, 8, 323, 128, 4.0, "random"),
    "e1": (3, 2, 1, 70, 32, 4.0, "random"),
    "e2_c32": (4, 2, 2, 192, 32, 4.0, "random"),
    "e5_c130": (5, 1, 5, 131, 130, 4.0, "random"),
    "e16": (6, 1, 16, 150, 128, 4.0, "random"),
    "e32": (7, 1, 32, 100, 40, 4.0, "random"),
    "l1": (8, 2, 8, 1, 16, 4.0, "random"),
    "c1": (9, 1, 8, 65, 1, 4.0, "random"),
    "ramp_up": (10, 1, 8, 517, 128, 30.0, "ramp_up"),
    "ramp_down": (11, 1, 8, 517, 128, 30.0, "ramp_down"),
    "peaked": (12, 2, 8, 260, 64, 40.0, "random"),
    "flat": (13, 1, 8, 200, 64, 4.0, "flat"),
    "select": (14, 2, 8, 256, 128, 0.0, "select"),
}
# Quantities whose reference is zero in exact arithmetic: judged by a norm ratio, not by a relative error.
ZERO_GRADS = {"flat": ("dq",), "l1": ("dq", "dk"), "select": ("dq", "dk")}


def attention(mono_q, mono_k, multi_v, dtype=torch.float64):
    """mono_q (n, L, E), mono_k (n, E, L), multi_v (n, C, L) -> (n, C, L): lines 362, 363 and 366 of the reference."""
    mono_q, mono_k, multi_v = mono_q.to(dtype), mono_k.to(dtype), multi_v.to(dtype)
    mono_score = torch.bmm(mono_q, mono_k)
    mono_atten = torch.softmax(mono_score, dim=-1)
    return torch.bmm(multi_v, mono_atten.permute(0, 2, 1))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def select_permutations(seed, n, L):
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.stack([torch.randperm(L, generator=g) for _ in range(n)])


def build_case(seed, n, E, L, C, amp, pattern):
    """q, k (n, E, L) and v, cotangent (n, C, L), float32, channel-major; mono_q of the reference is q.permute(0, 2, 1)."""
    g = torch.Generator().manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    if pattern == "select":
        assert L <= 2 ** E
        bits = ((torch.arange(L)[None, :] >> torch.arange(E)[:, None]) & 1).double() * 16.0 - 8.0  # (E, L): +-8 sign codes
        perm = select_permutations(seed, n, L)
        k = bits[None].repeat(n, 1, 1)
        q = torch.stack([bits[:, perm[b]] for b in range(n)])
        c, j = torch.arange(C)[:, None], torch.arange(L)[None, :]
        v = (((3 * c + 7 * j) % 11) - 5).double()[None].repeat(n, 1, 1)
        cot = torch.stack([(((5 * c + 3 * j + 2 * b) % 7) - 3).double() for b in range(n)])
    else:
        sigma = math.sqrt(amp) / E ** 0.25  # s = sum of E products of variance sigma^4: standard deviation amp
        q, k = randn(n, E, L) * sigma, randn(n, E, L) * sigma
        v, cot = randn(n, C, L), randn(n, C, L)
        if pattern in ("ramp_up", "ramp_down"):
            ramp = (torch.arange(L, dtype=torch.float64) - (L - 1) / 2) / 64.0  # in units of two key tiles
            k[:, 0, :] = (ramp if pattern == "ramp_up" else -ramp) * 1.5 * math.sqrt(amp)
            q[:, 0, :] = randn(n, L).abs() + math.sqrt(amp)
        elif pattern == "flat":
            k = k[:, :, :1].repeat(1, 1, L)
        else:
            assert pattern == "random", pattern
    f = lambda t: t.to(torch.float32).contiguous()
    return {"q": f(q), "k": f(k), "v": f(v), "cotangent": f(cot)}


def evaluate(fn, case, device=None, strided_q=True):
    """out, dq (n, E, L), dk, dv of fn(mono_q, mono_k, multi_v) at the case's cotangent; mono_q is the permuted view of q."""
    q, k, v = (case[key].clone() if device is None else case[key].to(device) for key in ("q", "k", "v"))
    q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    mono_q = q.permute(0, 2, 1) if strided_q else q.permute(0, 2, 1).contiguous()
    out = fn(mono_q, k, v)
    cot = case["cotangent"].to(out.device, out.dtype)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), cot)
    return {"out": out.detach(), "dq": dq, "dk": dk, "dv": dv}


@functools.lru_cache(maxsize=None)
def record(name):
    """A record of the fixtures: q, k, v, cotangent and the reference's out, dq, dk, dv."""
    with np.load(FIXTURES) as f:
        return {key: torch.from_numpy(f[f"{name}.{key}"]) for key in ("q", "k", "v", "cotangent", "out", "dq", "dk", "dv")}


@functools.lru_cache(maxsize=None)
def case_of(name):
    return record(name) if name in RECORDS else build_case(*CASES[name])


@functools.lru_cache(maxsize=None)
def restatement(name, dtype=torch.float64):
    """The five lines on the CPU in `dtype`, computed once per case and shared (do not write into it)."""
    return evaluate(lambda a, b, c: attention(a, b, c, dtype), case_of(name))


def bars(name):
    """Per quantity: max(FLOOR, 4 x what the float32 restatement loses on this case)."""
    r64, r32 = restatement(name, torch.float64), restatement(name, torch.float32)
    skip = ZERO_GRADS.get(name, ())
    return {key: max(FLOOR[key], 4.0 * rel_l2(r32[key], r64[key])) for key in FLOOR if key not in skip}
