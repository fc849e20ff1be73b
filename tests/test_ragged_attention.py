"""Ragged multi-head attention (pf3plat_amd.attention.ragged_attention, gsr_ragged_attention): every case of
tests/ragged_attention_ref.py against the float64 restatement of the reference's lines, within max(FLOOR, 4 x the float32 restatement's
own loss); the fences, the rotary sensitivity and the floors are checked on the CPU, where the argument checks and the C entry points'
refusals are checked too.  Cases of 64, 65 and 130 units take the kernel's unit search past its first trip of 64 (docs/PARITY.md
section 24.1); the CPU test states what each reaches."""
import ctypes
import os

import pytest
import torch

from pf3plat_amd import _lib, attention
from tests import ragged_attention_ref as ref

gpu = pytest.mark.gpu


# ---- CPU: the yardstick itself
def test_floors_are_of_the_size_of_the_worst_float32_loss():
    worst = {"out": 0.0, "lse": 0.0}
    for name in ref.ALL:
        loss = ref.float32_loss(name)
        print(name, {k: f"{v:.3e}" for k, v in loss.items()})
        worst = {k: max(worst[k], loss[k]) for k in worst}
    print("worst", worst)
    for key, floor in ref.FLOOR.items():
        assert worst[key] <= floor <= 2.0 * worst[key], (key, worst[key], floor)


def test_no_bar_is_above_the_cap():
    for name in ref.ALL:
        for key, bar in ref.bars(name).items():
            assert bar <= ref.CAP, (name, key, bar)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_fence_construction(name):
    """Rows next to every key range hold keys that outscore the unit's own by at least 100 and v of magnitude 1e3; q is NaN wherever no
    unit owns the row; the restatement over ranges one row too long differs from the true one by more than 1000 x the bar."""
    c = ref.case_of(name)
    T, qr, kr = c["T"], c["q_ranges"], c["k_ranges"]
    own = ref.owned_rows(T, qr)
    assert bool(torch.isnan(c["q"][~own]).all()) and not bool(torch.isnan(c["q"][own]).any())
    assert not bool(torch.isnan(c["k"]).any()) and not bool(torch.isnan(c["v"]).any())
    q, k = c["q"].double(), c["k"].double()
    if c["rot"] is not None:
        rot = c["rot"].double()
        q, k = ref.rotary(torch.nan_to_num(q), rot), ref.rotary(k, rot)
    checked = 0
    for (a, n), (b, m) in zip(qr, kr):
        if n == 0 or m == 0:
            continue
        own_max = (torch.einsum("ihd,jhd->hij", q[a:a + n], k[b:b + m]) * c["scale"]).amax()
        for row in (b - 1, b + m):
            if 0 <= row < T:
                fence = torch.einsum("ihd,hd->hi", q[a:a + n], k[row]) * c["scale"]
                assert float(fence.amin() - own_max) >= 100.0, (name, row)
                assert bool((c["v"][row].abs() == 1e3).all())
                checked += 1
    assert checked >= 1
    true = ref.restatement(name)[0]
    bar = ref.bars(name)["out"]
    wide = ref.attention(c["q"], c["k"], c["v"], qr, ref.widened(kr, T), c["scale"], c["rot"])[0]
    assert ref.owned_error(wide, true, own) > 1000.0 * bar
    if name != "blocks":  # (one unit: a query range cannot grow into anything but its own keys' rows; the sentinel test covers that)
        wide_q = ref.attention(torch.nan_to_num(c["q"], nan=1.0), c["k"], c["v"], ref.widened(qr, T), kr, c["scale"], c["rot"])[0]
        assert not torch.equal(wide_q[~own], true[~own])  # a query past a range lands on a row that must keep its sentinel


@pytest.mark.parametrize("name", list(ref.ROTARY))
def test_rotary_sensitivity(name):
    c = ref.case_of(name)
    own = ref.owned_rows(c["T"], c["q_ranges"])
    true, bar = ref.restatement(name)[0], ref.bars(name)["out"]
    args = (torch.nan_to_num(c["q"]), c["k"], c["v"], c["q_ranges"], c["k_ranges"], c["scale"])
    assert ref.owned_error(ref.attention(*args, None)[0], true, own) > 1000.0 * bar
    assert ref.owned_error(ref.attention(*args, c["rot"].flip(0))[0], true, own) > 1000.0 * bar


def test_many_unit_cases_take_the_unit_search_past_its_first_trip():
    """The kernel finds a workgroup's unit by a scan over the units' query-block counts, 64 units a trip, and carries the blocks of
    the trips before (rg_find in gsr_attention.h).  "u64" ends in one trip with its last block in the last lane; "u65" has the only
    block of its second trip in lane 0, behind a lane 63 without blocks; "u130" takes three trips with block-less units on both sides
    of either trip edge.  Everywhere a two-block unit lies before the edge, so that the carried count is not the unit count.  A search
    without the carry pairs the queries past unit 63 with the keys of the unit 64 before: that moves the result by far more than a bar."""
    step = ref.FIND_STEP
    with open(os.path.join(os.path.dirname(_lib.SRC), "gsr_attention.h")) as f:
        assert f"u0 < a.U; u0 += {step})" in f.read()  # the trip the cases are sized by is the source's
    want = {"u64": (64, [0]), "u65": (65, [0, 64]), "u130": (130, [0, 65, 129])}  # units; per trip the unit of its first block
    for name in ref.MANY_CASES:
        c = ref.case_of(name)
        form, sizes, H, D, with_rot, interleaved, _ = ref.CASES[name]
        qr, kr = c["q_ranges"], c["k_ranges"]
        units, trips = want[name[:-2] if name.endswith("d8") else name]
        got = ref.search_trips(qr)
        print(name, "units", len(qr), "rows", c["T"], "trips (first unit with a block, blocks carried in)", got)
        assert form == "general" and len(qr) == units and len(got) == -(-units // step) and H == 2 and c["T"] < 1000
        assert (D, with_rot, interleaved) == ((8, False, False) if name.endswith("d8") else (64, True, True))
        assert [first for first, _ in got] == trips
        for trip, (first, carried) in enumerate(got):
            assert (carried > 0 and carried != trip * step) or trip == 0  # what is carried is a block count, not the unit count
            assert qr[first][1] > 0
        assert qr[units - 1][1] > 0  # the last unit has queries: the last block of the call is found in the last trip
        assert all(q in (0, 1, 2, 3, 5) and k in (0, 1, 2, 4, 7) or (q, k) == ref.TWO_BLOCKS for q, k in sizes)
        assert sum((q, k) == ref.TWO_BLOCKS for q, k in sizes) == 1
        for edge in range(step, units, step):  # no blocks in the lanes at a trip's edge
            assert qr[edge - 1][1] == 0 and (edge + 1 >= units or qr[edge][1] == 0), (name, edge)
        if units > step:
            own, true, bar = ref.owned_rows(c["T"], qr), ref.restatement(name)[0], ref.bars(name)["out"]
            later = ref.owned_rows(c["T"], qr[step:])
            lost = ref.attention(c["q"], c["k"], c["v"], qr, ref.without_carry(kr), c["scale"], c["rot"])[0]
            assert torch.equal(lost[own & ~later], true[own & ~later])
            assert ref.owned_error(lost, true, own) > 1000.0 * bar and ref.owned_error(lost, true, later) > 1000.0 * bar
    assert ref.search_trips(ref.case_of("u64")["q_ranges"])[0][0] == 0 and ref.case_of("u64")["q_ranges"][63][1] > 0
    assert ref.case_of("u64")["q_ranges"][62][1] == 0  # (its last lane holds blocks behind a lane that holds none)
    assert ref.MANY_SIZES["u65"][10] == ref.TWO_BLOCKS and ref.MANY_SIZES["u130"][70] == ref.TWO_BLOCKS


def test_select_case_is_a_gather_in_exact_arithmetic():
    c = ref.case_of("select")
    seed, B, H, N, M, D = ref.STREAM_CASES["select"][:6]
    out = ref.restatement("select", torch.float32)[0]
    assert torch.equal(out[ref.owned_rows(c["T"], c["q_ranges"])], _select_expected(c, seed, B, H, N))


def _select_expected(c, seed, B, H, N):
    perm = ref.attention_ref.select_permutations(seed, B, H, N)  # (B, H, N): query i hits key perm[b, h, i]
    rows = []
    for b in range(B):
        vb = c["v"][c["k_ranges"][b][0]:c["k_ranges"][b][0] + N]  # (M, H, D)
        rows.append(torch.stack([vb[perm[b, h], h] for h in range(H)], 1))
    return torch.cat(rows)


# ---- CPU: the wrapper's checks and the C entry points' refusals
def test_python_checks_fire_before_the_library_loads(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))
    t = lambda *s: torch.zeros(*s)
    ok = [(0, 4)], [(4, 4)]
    for q, k, v, qr, kr, kw in (
            (t(8, 2), t(8, 2, 4), t(8, 2, 4), *ok, {}),
            (t(8, 2, 4), t(8, 2, 5), t(8, 2, 4), *ok, {}),
            (t(8, 2, 4), t(8, 2, 4), t(7, 2, 4), *ok, {}),
            (t(8, 2, 65), t(8, 2, 65), t(8, 2, 65), *ok, {}),
            (t(8, 2, 0), t(8, 2, 0), t(8, 2, 0), *ok, {}),
            (t(8, 2, 4), t(8, 2, 4), t(8, 2, 4), [(0, 9)], [(4, 4)], {}),
            (t(8, 2, 4), t(8, 2, 4), t(8, 2, 4), [(-1, 2)], [(4, 4)], {}),
            (t(8, 2, 4), t(8, 2, 4), t(8, 2, 4), [(0, 4)], [(4, 5)], {}),
            (t(8, 2, 4), t(8, 2, 4), t(8, 2, 4), [(0, 4)], [(4, 4), (0, 1)], {}),
            (t(8, 2, 4), t(8, 2, 4), t(8, 2, 4), [], [], {}),
            (t(8, 2, 4), t(8, 2, 4), t(8, 2, 4), [(0.5, 4)], [(4, 4)], {}),
            (t(8, 2, 4), t(8, 2, 4), t(8, 2, 4), *ok, {"scale": float("inf")}),
            (t(8, 2, 4), t(8, 2, 4), t(8, 2, 4), *ok, {"rot": t(2, 8, 3)}),
            (t(8, 2, 3), t(8, 2, 3), t(8, 2, 3), *ok, {"rot": t(2, 8, 3)}),
            (t(8, 2, 4).double(), t(8, 2, 4), t(8, 2, 4), *ok, {})):
        with pytest.raises(ValueError, match="ragged_attention"):
            attention.ragged_attention(q, k, v, qr, kr, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        attention.ragged_attention(t(8, 2, 4), t(8, 2, 4), t(8, 2, 4), *ok)


def test_entry_points_refuse_bad_sizes_by_host_arithmetic():
    """Every refusal with NULL operand pointers: nothing is dereferenced, nothing launched (no GPU here)."""
    lib = _lib.load()
    arr = lambda *v: (ctypes.c_int32 * len(v))(*v)
    good = dict(U=2, T=100, H=4, D=64, scale=0.125, qb=arr(0, 50), qc=arr(50, 50), kb=arr(50, 0), kc=arr(50, 50), rot=None)

    def call(**kw):
        a = {**good, **kw}
        sizes = lib.gsr_ragged_attention_scratch_bytes(a["U"], a["T"], a["H"], a["D"], a["qb"], a["qc"], a["kb"], a["kc"])
        rc = lib.gsr_ragged_attention(a["U"], a["T"], a["H"], a["D"], a["scale"], a["qb"], None, a["qc"], None, a["kb"], None, a["kc"], None,
                                      None, None, None, None, None, None, a["rot"], None, None, None, None)
        return sizes, rc

    assert call() == (16, -1)  # sizes the call accepts; refused for its NULL pointers alone
    assert lib.gsr_ragged_attention_scratch_bytes(2, 100, 4, 33, good["qb"], good["qc"], good["kb"], good["kc"]) == 16
    for bad in (dict(U=0), dict(T=0), dict(H=0), dict(D=0), dict(D=65), dict(qc=arr(50, 51)), dict(kb=arr(50, 51)), dict(qb=arr(-1, 50)),
                dict(kc=arr(50, -1)), dict(T=1 << 20, H=64, D=64), dict(qb=None), dict(kc=None)):
        assert call(**bad) == (0, -1), bad
    assert call(scale=float("nan"))[1] == -1 and call(scale=float("inf"))[1] == -1
    one = ctypes.c_void_p(8)  # (never dereferenced: the sizes are refused first)
    assert call(D=33, rot=one)[1] == -1
    assert {"gsr_ragged_attention", "gsr_ragged_attention_scratch_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    assert lib.gsr_abi_version() == 5


# ---- GPU
def _run(name, device="cuda"):
    c = ref.case_of(name)
    if c["q"].is_contiguous():
        q, k, v = (c[key].to(device) for key in ("q", "k", "v"))
    else:  # the interleaved layout, kept: one (T, H, D, 3) buffer and its three views
        base = torch.stack([c["q"], c["k"], c["v"]], -1).to(device)
        q, k, v = base[..., 0], base[..., 1], base[..., 2]
        assert q.stride() == (3 * c["H"] * c["D"], 3 * c["D"], 3)
    rot = None if c["rot"] is None else c["rot"].to(device)
    out = torch.full((c["T"], c["H"], c["D"]), ref.SENTINEL, device=device)
    res, lse = attention.ragged_attention(q, k, v, c["q_ranges"], c["k_ranges"], c["scale"], rot, out=out, return_lse=True)
    assert res is out
    return out, lse


@gpu
@pytest.mark.parametrize("name", list(ref.ALL))
def test_matches_the_float64_restatement(name):
    c = ref.case_of(name)
    own = ref.owned_rows(c["T"], c["q_ranges"])
    out, lse = _run(name)
    torch.cuda.synchronize()
    r_out, r_lse = ref.restatement(name)
    bars = ref.bars(name)
    err = {"out": ref.owned_error(out, r_out, own), "lse": ref.owned_error(lse, r_lse, own)}
    print(name, {k: f"{v:.3e}" for k, v in err.items()}, {k: f"{v:.3e}" for k, v in bars.items()})
    # rows no unit owns keep the sentinel; units without keys are zeros and -inf exactly
    assert bool((out.cpu()[~own] == ref.SENTINEL).all())
    for (a, n), (_, m) in zip(c["q_ranges"], c["k_ranges"]):
        if n and not m:
            assert bool((out[a:a + n] == 0).all()) and bool((lse[:, a:a + n] == float("-inf")).all())
    assert not bool(torch.isnan(out).any())
    for key in err:
        assert err[key] <= bars[key], (name, key, err[key], bars[key])
    again, lse2 = _run(name)
    assert torch.equal(again, out) and torch.equal(lse2[:, own.to(lse2.device)], lse[:, own.to(lse.device)])  # the same bits on every call


@gpu
def test_select_is_the_gathered_v_bit_for_bit():
    c = ref.case_of("select")
    seed, B, H, N = ref.STREAM_CASES["select"][:4]
    out, _ = _run("select")
    assert torch.equal(out.cpu()[ref.owned_rows(c["T"], c["q_ranges"])], _select_expected(c, seed, B, H, N))


@gpu
def test_default_scale_and_fresh_output():
    """Without `out` and `scale`: D ** -0.5, and zeros where no unit owns the row."""
    c = ref.case_of("w34")
    base = torch.stack([c["q"], c["k"], c["v"]], -1).cuda()
    out = attention.ragged_attention(base[..., 0], base[..., 1], base[..., 2], c["q_ranges"], c["k_ranges"], rot=c["rot"].cuda())
    own = ref.owned_rows(c["T"], c["q_ranges"])
    assert out.is_contiguous() and bool((out.cpu()[~own] == 0).all())
    assert ref.owned_error(out, ref.restatement("w34")[0], own) <= ref.bars("w34")["out"]
