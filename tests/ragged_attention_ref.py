"""The yardstick of the ragged attention tests: per unit softmax(scale q' k'^T) v with the reference's rotary lines (reference
src/model/LightGlue/lightglue/lightglue.py:51-58, 106-130) restated as a torch function with a dtype switch - float64 is the reference,
float32 measures what the reference's own arithmetic loses -, the seeded cases with their fences, and the bars.  CPU only."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import attention_ref
from tests.attention_ref import rel_l2, rotate_half  # noqa: F401

CAP = 1e-4  # no bar of a test is above this
# What the float32 restatement loses against float64 at worst over CASES (rel-L2 over the owned rows; measured on the CPU by
# tests/test_ragged_attention.py::test_floors_are_of_the_size_of_the_worst_float32_loss, which prints it; rounded up in the second
# digit): the floor of the bars of the GPU tests.
FLOOR = {"out": 5.7e-6, "lse": 1.6e-7}
SENTINEL = 7.5  # what the tests write into `out` before a call: rows no unit owns keep it

# The six units of the issue as (q_count, k_count), laid out q range, k range, q range, ... without gaps: 871 rows.
SIX = ((70, 150), (0, 33), (1, 77), (45, 0), (131, 323), (40, 1))
# name: (form, sizes, H, D, with rot, interleaved layout, seed).  Forms: "general" - every unit a query range and a key range of its
# own, no gaps (at a query row k and v hold the fence, at a key row q holds NaN); "self" - the key range is the query range, one
# unowned fence row between units; "cross" - lists (m, n), two units per list with swapped partners, fence rows between ranges.
FIND_STEP = 64  # units a trip of the kernel's unit search (rg_find) takes; a query block is 128 rows
TWO_BLOCKS = (130, 40)  # a unit of two query blocks: after it the search's running block count is no longer the unit count


def many_units(count, seed, two_blocks_at, without_queries, with_queries):
    """`count` units with (queries, keys) drawn from {0, 1, 2, 3, 5} x {0, 1, 2, 4, 7}, the unit `two_blocks_at` TWO_BLOCKS, the units
    `without_queries` (0, keys) - they sit at the edges of a trip of the search -, the units `with_queries` at least (1, keys)."""
    g = torch.Generator().manual_seed(seed)
    nq = torch.tensor([0, 1, 2, 3, 5])[torch.randint(0, 5, (count,), generator=g)].tolist()
    nk = torch.tensor([0, 1, 2, 4, 7])[torch.randint(0, 5, (count,), generator=g)].tolist()
    for u in without_queries:
        nq[u] = 0
    for u in with_queries:
        nq[u] = max(nq[u], 1)
    nq[two_blocks_at], nk[two_blocks_at] = TWO_BLOCKS
    return tuple(zip(nq, nk))


# More units than one trip of the search: name: (units, seed of the counts, the two-block unit, units without queries, units with).
# "u64": one trip, the last block in the last lane; "u65": the only block of the second trip in its lane 0, behind an empty lane 63 and
# a two-block unit in the first trip; "u130": three trips, empty units on both sides of 63 | 64 and 127 | 128, a two-block unit in
# the second trip, the last unit with queries.
MANY = {
    "u64": (64, 21, 10, (62,), (0, 63)),
    "u65": (65, 22, 10, (63,), (0, 64)),
    "u130": (130, 23, 70, (63, 64, 127, 128), (0, 65, 129)),
}
MANY_SIZES = {name: many_units(*spec) for name, spec in MANY.items()}

CASES = {
    "w64": ("general", SIX, 4, 64, True, True, 1),
    "w63": ("general", SIX, 3, 63, False, False, 2),
    "w62": ("general", SIX, 1, 62, True, False, 3),
    "w34": ("general", SIX, 3, 34, True, True, 4),
    "w33": ("general", SIX, 1, 33, False, True, 5),
    "w32": ("general", SIX, 4, 32, True, False, 6),
    "w2": ("general", SIX, 3, 2, True, True, 7),
    "w1": ("general", SIX, 1, 1, False, False, 8),
    "blocks": ("general", ((260, 517),), 3, 64, True, True, 9),  # more than two query blocks, 17 key tiles
    "self": ("self", (70, 131, 0, 1, 45), 4, 64, True, True, 10),
    "cross": ("cross", ((70, 150), (45, 0), (1, 77), (131, 40)), 4, 64, False, False, 11),
    "u64": ("general", MANY_SIZES["u64"], 2, 64, True, True, 31),
    "u65": ("general", MANY_SIZES["u65"], 2, 64, True, True, 32),
    "u130": ("general", MANY_SIZES["u130"], 2, 64, True, True, 33),
    "u65d8": ("general", MANY_SIZES["u65"], 2, 8, False, False, 34),
    "u130d8": ("general", MANY_SIZES["u130"], 2, 8, False, False, 35),
}
MANY_CASES = tuple(n for n in CASES if n.startswith("u"))
# The online-softmax constructions of tests/attention_ref.py at D = 64: (seed, B, H, N, M, D, amp, pattern, scale); a batch entry is a unit.
STREAM_CASES = {
    "ramp_up": (9, 1, 2, 260, 517, 64, 30.0, "ramp_up", None),
    "ramp_down": (10, 1, 2, 260, 517, 64, 30.0, "ramp_down", None),
    "peaked": (11, 2, 2, 130, 260, 64, 40.0, "random", None),
    "select": (12, 2, 3, 256, 256, 64, 0.0, "select", 0.5),
}
ALL = tuple(CASES) + tuple(STREAM_CASES)
ROTARY = tuple(n for n, c in CASES.items() if c[4])


def rotary(x, rot):
    """apply_cached_rotary_emb (lightglue.py:57-58) on packed rows: x (T, H, D), rot (2, T, D)."""
    return (x * rot[0][:, None, :]) + (rotate_half(x) * rot[1][:, None, :])


def unrotate(y, rot):
    """x with rotary(x, rot) = y, float64: per pair the inverse of [[c0, -s0], [s1, c1]]."""
    c, s = rot[0][:, None, :].unflatten(-1, (-1, 2)), rot[1][:, None, :].unflatten(-1, (-1, 2))
    y = y.unflatten(-1, (-1, 2))
    c0, c1, s0, s1, y0, y1 = c[..., 0], c[..., 1], s[..., 0], s[..., 1], y[..., 0], y[..., 1]
    det = c0 * c1 + s0 * s1
    return torch.stack(((c1 * y0 + s0 * y1) / det, (c0 * y1 - s1 * y0) / det), -1).flatten(-2)


def attention(q, k, v, q_ranges, k_ranges, scale, rot=None, dtype=torch.float64, fill=SENTINEL):
    """q, k, v (T, H, D) -> out (T, H, D), lse (H, T): rows no unit owns hold `fill` (lse: NaN).  Reads nothing outside the ranges."""
    T, H, D = q.shape
    out = torch.full((T, H, D), fill, dtype=dtype)
    lse = torch.full((H, T), float("nan"), dtype=dtype)
    rot = None if rot is None else rot.to(dtype)
    for (qb, qc), (kb, kc) in zip(q_ranges, k_ranges):
        if qc == 0:
            continue
        if kc == 0:  # Attention.forward, lightglue.py:107-108
            out[qb:qb + qc], lse[:, qb:qb + qc] = 0.0, -math.inf
            continue
        qu, ku, vu = q[qb:qb + qc].to(dtype), k[kb:kb + kc].to(dtype), v[kb:kb + kc].to(dtype)
        if rot is not None:
            qu, ku = rotary(qu, rot[:, qb:qb + qc]), rotary(ku, rot[:, kb:kb + kc])
        sim = torch.einsum("ihd,jhd->hij", qu, ku) * scale
        out[qb:qb + qc] = torch.einsum("hij,jhd->ihd", F.softmax(sim, -1), vu)
        lse[:, qb:qb + qc] = torch.logsumexp(sim, -1)
    return out, lse


def layout(form, sizes):
    """-> T, q_ranges, k_ranges, fence rows (unowned rows between ranges; empty in the general form)."""
    qr, kr, fence, t = [], [], [], 0
    if form == "general":
        for nq, nk in sizes:
            qr.append((t, nq))
            kr.append((t + nq, nk))
            t += nq + nk
    elif form == "self":
        for n in sizes:
            fence.append(t)
            qr.append((t + 1, n))
            kr.append((t + 1, n))
            t += 1 + n
        fence.append(t)
        t += 1
    else:
        assert form == "cross", form
        for m, n in sizes:
            fence.append(t)
            a, b = (t + 1, m), (t + 2 + m, n)
            fence.append(t + 1 + m)
            qr += [a, b]
            kr += [b, a]
            t += 2 + m + n
        fence.append(t)
        t += 1
    return t, tuple(qr), tuple(kr), tuple(fence)


def owned_rows(T, q_ranges):
    own = torch.zeros(T, dtype=torch.bool)
    for b, c in q_ranges:
        own[b:b + c] = True
    return own


def key_rows(T, q_ranges, k_ranges):
    """The rows some unit WITH QUERIES reads as keys: every other row of k and v is fence."""
    return owned_rows(T, [kr for qr, kr in zip(q_ranges, k_ranges) if qr[1] > 0])


def widened(ranges, T):
    """Every non-empty range one row longer on either side, inside [0, T]: what a kernel that overruns a range would read."""
    return tuple((max(b - 1, 0), min(b + c + 1, T) - max(b - 1, 0)) if c else (b, c) for b, c in ranges)


def search_trips(q_ranges):
    """Per trip of the unit search over FIND_STEP units: (the unit that holds the trip's first query block or None, the query blocks
    of the units before the trip - what the search carries into it)."""
    blocks = [(c + 127) // 128 for _, c in q_ranges]
    out = []
    for u0 in range(0, len(blocks), FIND_STEP):
        first = next((u for u in range(u0, min(u0 + FIND_STEP, len(blocks))) if blocks[u]), None)
        out.append((first, sum(blocks[:u0])))
    return out


def without_carry(k_ranges):
    """The key ranges a search that forgot its carried count would pair the queries with: a unit past the first trip attends the keys of
    the unit FIND_STEP before it."""
    return tuple(k_ranges[u - FIND_STEP] if u >= FIND_STEP else k_ranges[u] for u in range(len(k_ranges)))


@functools.lru_cache(maxsize=None)
def case_of(name):
    """-> dict: q, k, v (T, H, D) float32 views of the case's layout, rot (2, T, D) or None, the ranges, scale, T, H, D."""
    if name in STREAM_CASES:
        seed, B, H, N, M, D, amp, pattern, scale = STREAM_CASES[name]
        c = attention_ref.build_case(seed, B, H, N, M, D, amp, pattern, scale)
        T, qr, kr, _ = layout("general", ((N, M),) * B)
        q, k, v = (torch.zeros(T, H, D) for _ in range(3))
        for b in range(B):
            q[qr[b][0]:qr[b][0] + N] = c["q"][b].transpose(0, 1)
            k[kr[b][0]:kr[b][0] + M] = c["k"][b].transpose(0, 1)
            v[kr[b][0]:kr[b][0] + M] = c["v"][b].transpose(0, 1)
        return {"q": q, "k": k, "v": v, "rot": None, "q_ranges": qr, "k_ranges": kr, "scale": D ** -0.5 if scale is None else scale,
                "T": T, "H": H, "D": D, "fenced": False, "seed": seed}
    form, sizes, H, D, with_rot, interleaved, seed = CASES[name]
    T, qr, kr, fence = layout(form, sizes)
    g = torch.Generator().manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    scale = D ** -0.5
    # q' and k', the operands as the score product sees them: normal with variance 4 (the scores have standard deviation 4), and in
    # q' a first channel of at least 2 that the fence keys answer
    qp, kp, v = randn(T, H, D) * 2.0, randn(T, H, D) * 2.0, randn(T, H, D)
    qp[..., 0] = randn(T, H).abs() + 2.0
    is_q, is_k = owned_rows(T, qr), key_rows(T, qr, kr)
    rot = None
    if with_rot:  # per token and pair an angle; cosines and sines each repeated twice as the encoding gives them, then 2 % apart
        ang = torch.rand(T, D // 2, generator=g, dtype=torch.float64) * (2 * math.pi)
        rot = torch.stack([torch.cos(ang), torch.sin(ang)]).repeat_interleave(2, dim=-1) * (1.0 + 0.02 * randn(2, T, D))
    own_max = max(float((torch.einsum("ihd,jhd->hij", qp[a:a + n], kp[b:b + m]) * scale).max()) for (a, n), (b, m) in zip(qr, kr) if n and m)
    big = (own_max + 120.0) / (scale * 2.0)  # a fence key scores at least own_max + 120 against every query
    fence_k = ~is_k
    kp[fence_k] = 0.0
    kp[fence_k, :, 0] = big
    v[fence_k] = torch.where(torch.arange(D) % 2 == 0, 1e3, -1e3).to(torch.float64)
    q, k = (unrotate(qp, rot), unrotate(kp, rot)) if with_rot else (qp, kp)
    q[~is_q] = float("nan")
    f = lambda t: t.to(torch.float32)
    if interleaved:  # the Wqkv output: (T, 3 H D) viewed as (T, H, D, 3)
        base = torch.stack([f(q), f(k), f(v)], -1).contiguous()
        q32, k32, v32 = base[..., 0], base[..., 1], base[..., 2]
    else:
        q32, k32, v32 = f(q).contiguous(), f(k).contiguous(), f(v).contiguous()
    return {"q": q32, "k": k32, "v": v32, "rot": None if rot is None else f(rot).contiguous(), "q_ranges": qr, "k_ranges": kr,
            "scale": scale, "T": T, "H": H, "D": D, "fenced": True, "fence_rows": fence, "seed": seed}


@functools.lru_cache(maxsize=None)
def restatement(name, dtype=torch.float64):
    """(out, lse) of the case on the CPU in `dtype`, computed once and shared (do not write into it)."""
    c = case_of(name)
    return attention(c["q"], c["k"], c["v"], c["q_ranges"], c["k_ranges"], c["scale"], c["rot"], dtype)


def owned_error(a, b, own):
    """rel-L2 over the rows `own` of two (T, H, D) or (H, T) arrays, rows with -inf in b required equal and left out."""
    a, b = a.double().cpu(), b.double().cpu()
    if a.dim() == 2:
        a, b = a.transpose(0, 1), b.transpose(0, 1)
    a, b = a[own], b[own]
    inf = torch.isinf(b)
    assert bool((a[inf] == b[inf]).all())
    return rel_l2(a[~inf], b[~inf]) if bool((~inf).any()) else 0.0


def float32_loss(name):
    c = case_of(name)
    own = owned_rows(c["T"], c["q_ranges"])
    r64, r32 = restatement(name, torch.float64), restatement(name, torch.float32)
    return {"out": owned_error(r32[0], r64[0], own), "lse": owned_error(r32[1], r64[1], own)}


def bars(name):
    """Per quantity: max(FLOOR, 4 x what the float32 restatement loses on this case)."""
    loss = float32_loss(name)
    return {key: max(FLOOR[key], 4.0 * loss[key]) for key in FLOOR}
