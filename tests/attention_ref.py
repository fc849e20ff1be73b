"""The yardstick of the multi-head attention tests: the attention of LightGlue's blocks (reference
src/model/LightGlue/lightglue/lightglue.py:57-58, 106-130, 133-224), the rotary embedding and both blocks restated as torch functions
with a dtype switch - float64 is the reference, float32 measures what the reference's own arithmetic loses -, the seeded cases, the
records of the reference's own classes (tests/golden/make_attention_fixtures.py) and rel_l2.  CPU only."""
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# name: (file, kind, embed_dim, heads, B, N, M, with encoding, seed).  The cross record is a file of its own: a committed file stays under 1 MiB.
RECORDS = {
    "self_rot": ("attention_fixtures.npz", "self", 64, 2, 2, 70, 70, True, 101),
    "self_plain": ("attention_fixtures.npz", "self", 24, 3, 2, 45, 45, False, 102),
    "cross": ("attention_fixtures_cross.npz", "cross", 64, 2, 2, 70, 150, False, 103),
}

CAP = 1e-4  # no bar of a test is above this
# What the float32 restatement loses against float64 at worst over CASES (rel-L2; measured on the CPU by
# tests/test_attention.py::test_bars_stay_under_the_cap, which prints it; rounded up in the second digit): the floor of the bars of the GPU tests.
FLOOR = {"out": 5.1e-6, "dq": 2.2e-5, "dk": 1.9e-5, "dv": 5.3e-6}
# ... and what the float32 restatement of a BLOCK loses at worst over the records, over every output, input gradient and parameter
# gradient (test_module_floor_is_the_worst_float32_loss prints it): the floor of the module-level bars.
MODULE_FLOOR = 1.4e-6

# name: (seed, B, H, N, M, D, amp, pattern, scale).  scale None is D ** -0.5.  q and k are normal with variance amp: the scores,
# D ** -0.5 times sums of D products, have standard deviation amp unless the pattern says otherwise.
CASES = {
    "d32": (1, 2, 4, 131, 131, 32, 4.0, "random", None),
    "cross": (2, 2, 2, 70, 323, 32, 4.0, "random", None),
    "cross_wide": (3, 1, 3, 323, 70, 8, 4.0, "random", None),
    "d1": (4, 2, 2, 70, 45, 1, 4.0, "random", None),
    "d5": (5, 1, 3, 131, 200, 5, 4.0, "random", None),
    "d31": (6, 1, 2, 100, 150, 31, 4.0, "random", None),
    "n1": (7, 2, 2, 1, 77, 16, 4.0, "random", None),
    "m1": (8, 2, 2, 40, 1, 16, 4.0, "random", None),
    "ramp_up": (9, 1, 2, 260, 517, 32, 30.0, "ramp_up", None),
    "ramp_down": (10, 1, 2, 260, 517, 32, 30.0, "ramp_down", None),
    "peaked": (11, 2, 2, 130, 260, 32, 40.0, "random", None),
    "select": (12, 2, 3, 256, 256, 8, 0.0, "select", 0.5),
}
# Quantities whose reference is zero in exact arithmetic: judged by a norm ratio, not by a relative error.
ZERO_GRADS = {"m1": ("dq", "dk"), "select": ("dq", "dk")}
ZERO_RATIO = 1e-5


def scale_of(name):
    s = None if name.startswith("rec_") else CASES[name][8]
    return case_of(name)["q"].shape[-1] ** -0.5 if s is None else s


def attention(q, k, v, scale=None, dtype=torch.float64):
    """q (B, H, N, D), k, v (B, H, M, D) -> (B, H, N, D): lightglue.py:125-130 without a mask."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    s = q.shape[-1] ** -0.5 if scale is None else scale
    sim = torch.einsum("...id,...jd->...ij", q, k) * s
    return torch.einsum("...ij,...jd->...id", F.softmax(sim, -1), v)


def probabilities(q, k, scale=None, dtype=torch.float64):
    s = q.shape[-1] ** -0.5 if scale is None else scale
    sim = torch.einsum("...id,...jd->...ij", q.to(dtype), k.to(dtype)) * s
    return sim, F.softmax(sim, -1)


def bidirectional(qk0, qk1, v0, v1, scale, dtype=torch.float64):
    """lightglue.py:210-217 as the reference writes them: sqrt(scale) on either side, one similarity, two softmaxes."""
    qk0, qk1, v0, v1 = (t.to(dtype) for t in (qk0, qk1, v0, v1))
    qk0, qk1 = qk0 * scale ** 0.5, qk1 * scale ** 0.5
    sim = torch.einsum("bhid, bhjd -> bhij", qk0, qk1)
    attn01 = F.softmax(sim, dim=-1)
    attn10 = F.softmax(sim.transpose(-2, -1).contiguous(), dim=-1)
    m0 = torch.einsum("bhij, bhjd -> bhid", attn01, v1)
    m1 = torch.einsum("bhji, bhjd -> bhid", attn10.transpose(-2, -1), v0)
    return m0, m1


def rotate_half(x):
    x = x.unflatten(-1, (-1, 2))
    x1, x2 = x.unbind(dim=-1)
    return torch.stack((-x2, x1), dim=-1).flatten(start_dim=-2)


def apply_cached_rotary_emb(freqs, t):
    return (t * freqs[0]) + (rotate_half(t) * freqs[1])


def _ffn(p, x):
    h = F.linear(x, p["ffn.0.weight"], p["ffn.0.bias"])
    h = F.gelu(F.layer_norm(h, (h.shape[-1],), p["ffn.1.weight"], p["ffn.1.bias"]))
    return F.linear(h, p["ffn.3.weight"], p["ffn.3.bias"])


def self_block(p, heads, x, encoding=None, attn=None):
    """SelfBlock.forward (lightglue.py:158-166) over a dict of parameters; returns the output and (q, k, v, context)."""
    qkv = F.linear(x, p["Wqkv.weight"], p["Wqkv.bias"]).unflatten(-1, (heads, -1, 3)).transpose(1, 2)
    q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
    if encoding is not None:
        q, k = apply_cached_rotary_emb(encoding, q), apply_cached_rotary_emb(encoding, k)
    context = attention(q, k, v, dtype=q.dtype) if attn is None else attn(q, k, v)
    message = F.linear(context.transpose(1, 2).flatten(start_dim=-2), p["out_proj.weight"], p["out_proj.bias"])
    return x + _ffn(p, torch.cat([x, message], -1)), (q, k, v, context)


def cross_block(p, heads, x0, x1, both=None):
    """CrossBlock.forward (lightglue.py:198-224), the einsum path; returns (x0', x1') and (qk0, qk1, v0, v1, m0, m1)."""
    scale = (x0.shape[-1] // heads) ** -0.5
    split = lambda t: t.unflatten(-1, (heads, -1)).transpose(1, 2)
    qk0, qk1 = (split(F.linear(x, p["to_qk.weight"], p["to_qk.bias"])) for x in (x0, x1))
    v0, v1 = (split(F.linear(x, p["to_v.weight"], p["to_v.bias"])) for x in (x0, x1))
    m0, m1 = bidirectional(qk0, qk1, v0, v1, scale, qk0.dtype) if both is None else both(qk0, qk1, v0, v1, scale)
    o0, o1 = (F.linear(m.transpose(1, 2).flatten(start_dim=-2), p["to_out.weight"], p["to_out.bias"]) for m in (m0, m1))
    return (x0 + _ffn(p, torch.cat([x0, o0], -1)), x1 + _ffn(p, torch.cat([x1, o1], -1))), (qk0, qk1, v0, v1, m0, m1)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def select_permutations(seed, B, H, L):
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.stack([torch.randperm(L, generator=g) for _ in range(B * H)]).reshape(B, H, L)


def build_case(seed, B, H, N, M, D, amp, pattern, scale=None):
    """q (B, H, N, D), k, v (B, H, M, D), cotangent (B, H, N, D), float32, contiguous."""
    g = torch.Generator().manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    if pattern == "select":
        # +-8 sign codes of the key index: with scale 0.5 the score is 256 on the hit and at most 192 elsewhere, so every other weight is
        # at most exp(-64) = 2^-92 - below half an ulp of any non-zero small integer: v and the cotangent avoid zero, and p v IS v[hit]
        assert N == M and M <= 2 ** D and scale == 0.5
        bits = ((torch.arange(M)[:, None] >> torch.arange(D)[None, :]) & 1).double() * 16.0 - 8.0  # (M, D)
        perm = select_permutations(seed, B, H, M)
        k = bits[None, None].repeat(B, H, 1, 1)
        q = bits[perm]  # (B, H, N, D): query i hits key perm[b, h, i]
        hd, j, c = torch.arange(H)[:, None, None], torch.arange(M)[None, :, None], torch.arange(D)[None, None, :]
        sign = 1.0 - 2.0 * ((j + c) % 2)
        v = ((((3 * c + 7 * j + 2 * hd) % 5) + 1) * sign).double()[None].repeat(B, 1, 1, 1)
        cot = torch.stack([(((5 * c + 3 * j + 2 * b + hd) % 6) + 1) * sign for b in range(B)]).double()
    else:
        sigma = math.sqrt(amp)  # s = D^-1/2 times a sum of D products of variance sigma^4: standard deviation amp
        q, k = randn(B, H, N, D) * sigma, randn(B, H, M, D) * sigma
        v, cot = randn(B, H, M, D), randn(B, H, N, D)
        if pattern in ("ramp_up", "ramp_down"):
            ramp = (torch.arange(M, dtype=torch.float64) - (M - 1) / 2) / 64.0  # in units of two key tiles
            k[..., 0] = (ramp if pattern == "ramp_up" else -ramp) * 1.25 * math.sqrt(amp) * math.sqrt(D)  # (sqrt(D): the scale cancels)
            q[..., 0] = randn(B, H, N).abs() + math.sqrt(amp)
        else:
            assert pattern == "random", pattern
    f = lambda t: t.to(torch.float32).contiguous()
    return {"q": f(q), "k": f(k), "v": f(v), "cotangent": f(cot)}


def evaluate(fn, case, device=None):
    """out, dq, dk, dv (all (B, H, tokens, D)) of fn(q, k, v) at the case's cotangent."""
    q, k, v = (case[key].clone() if device is None else case[key].to(device) for key in ("q", "k", "v"))
    q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    out = fn(q, k, v)
    cot = case["cotangent"].to(out.device, out.dtype)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), cot)
    return {"out": out.detach(), "dq": dq, "dk": dk, "dv": dv}


def record_inputs(name):
    """The seeded inputs and cotangents of a record (not stored in the fixtures: they are what goes INTO the reference).  Self:
    x, positions (with encoding), cot; cross: x0, x1, cot0, cot1."""
    _, kind, E, _, B, N, M, with_enc, seed = RECORDS[name]
    g = torch.Generator().manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(torch.float32)
    if kind == "self":
        d = {"x": randn(B, N, E), "cot": randn(B, N, E)}
        if with_enc:
            d["positions"] = torch.rand(B, N, 2, generator=g, dtype=torch.float64).to(torch.float32) * 2 - 1
        return d
    return {"x0": randn(B, N, E), "x1": randn(B, M, E), "cot0": randn(B, N, E), "cot1": randn(B, M, E)}


@functools.lru_cache(maxsize=None)
def record(name):
    """A record of the fixtures: everything the reference's own class computed, by name (state.*, grad.*, out*, dx*, the hooked q, k, v
    and context, for self_rot the encoding and its gradient), plus the seeded inputs."""
    with np.load(os.path.join(GOLDEN, RECORDS[name][0])) as f:
        d = {key[len(name) + 1:]: torch.from_numpy(f[key]) for key in f.files if key.startswith(name + ".")}
    d.update(record_inputs(name))
    return d


def state_of(name):
    return {k[len("state."):]: v for k, v in record(name).items() if k.startswith("state.")}


def kernel_records():
    """The kernel-level records: name -> q, k, v and the reference's context, as the hooks saw them."""
    out = {}
    for name in ("self_rot", "self_plain"):
        r = record(name)
        out["rec_" + name] = {"q": r["q"], "k": r["k"], "v": r["v"], "context": r["context"]}
    r = record("cross")
    out["rec_cross_m0"] = {"q": r["qk0"], "k": r["qk1"], "v": r["v1"], "context": r["m0"]}
    out["rec_cross_m1"] = {"q": r["qk1"], "k": r["qk0"], "v": r["v0"], "context": r["m1"]}
    return out


def _record_cotangent(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(torch.float32)


@functools.lru_cache(maxsize=None)
def case_of(name):
    if name.startswith("rec_"):
        r = kernel_records()[name]
        return {"q": r["q"].contiguous(), "k": r["k"].contiguous(), "v": r["v"].contiguous(),
                "cotangent": _record_cotangent(r["q"].shape, 500 + len(name))}
    return build_case(*CASES[name])


KERNEL_RECORDS = ("rec_self_rot", "rec_self_plain", "rec_cross_m0", "rec_cross_m1")


@functools.lru_cache(maxsize=None)
def restatement(name, dtype=torch.float64):
    """The attention on the CPU in `dtype`, computed once per case and shared (do not write into it)."""
    return evaluate(lambda a, b, c: attention(a, b, c, scale_of(name), dtype), case_of(name))


def bars(name):
    """Per quantity: max(FLOOR, 4 x what the float32 restatement loses on this case)."""
    r64, r32 = restatement(name, torch.float64), restatement(name, torch.float32)
    skip = ZERO_GRADS.get(name, ())
    return {key: max(FLOOR[key], 4.0 * rel_l2(r32[key], r64[key])) for key in FLOOR if key not in skip}


def run_block(name, dtype=torch.float64, device=None, module=None, need_x1=True):
    """A record's block at the record's weights, inputs and cotangents: the restatement in `dtype`, or `module` (the class under test,
    already holding the state) on `device`.  Returns name -> tensor: out / out0, out1, dx / dx0, dx1, denc, grad.<parameter>."""
    _, kind, _, heads, *_ = RECORDS[name]
    r = record(name)
    to = lambda t: t.to(dtype if module is None else torch.float32).to(device or "cpu")
    res = {}
    if module is None:
        params = {k: to(v).requires_grad_(True) for k, v in state_of(name).items()}
        plist = list(params.items())
    else:
        plist = list(module.named_parameters())
    if kind == "self":
        x = to(r["x"]).requires_grad_(True)
        enc = to(r["encoding"]).requires_grad_(True) if "encoding" in r else None
        out = self_block(params, heads, x, enc)[0] if module is None else module(x, enc)
        wrt = [x] + ([enc] if enc is not None else []) + [p for _, p in plist]
        grads = torch.autograd.grad(out, wrt, to(r["cot"]))
        res["out"], res["dx"] = out.detach(), grads[0]
        if enc is not None:
            res["denc"] = grads[1]
        pg = grads[len(wrt) - len(plist):]
    else:
        x0, x1 = to(r["x0"]).requires_grad_(True), to(r["x1"]).requires_grad_(True)
        if module is None:
            o0, o1 = cross_block(params, heads, x0, x1)[0]
        else:
            o0, o1 = module(x0, x1, need_x1=need_x1)
        wrt = [x0, x1] + [p for _, p in plist]
        if need_x1:
            grads = torch.autograd.grad([o0, o1], wrt, [to(r["cot0"]), to(r["cot1"])])
            res["out1"] = o1.detach()
        else:
            grads = torch.autograd.grad(o0, wrt, to(r["cot0"]), allow_unused=True)
        res["out0"], res["dx0"], res["dx1"] = o0.detach(), grads[0], grads[1]
        pg = grads[2:]
    for (n, _), gr in zip(plist, pg):
        res["grad." + n] = gr
    return res


@functools.lru_cache(maxsize=None)
def block_restatement(name, dtype=torch.float64):
    return run_block(name, dtype)
