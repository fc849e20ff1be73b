"""Match assignment on the device (pf3plat_amd.matching; gsr_match_assignment; definition: include/gsr.h) against
tests/match_ref.py - the reference's lines restated, float64 the yardstick - and against the records of the reference's own
MatchAssignment and filter_matches, tests/golden/match_fixtures.npz.

Bars (docs/PARITY.md section 21, conventions of sections 18 and 20): every index - matches0, matches1, the compact idx0 / idx1,
count, ids_i / ids_j - EQUALS the float64 restatement's on every keypoint of every case; that is a fair demand because every case
keeps its decisions GAP away from rounding (test_cases_meet_their_conditions).  Scores lie within max(FLOOR, 4 x |float32
restatement - float64 restatement|) rel-L2 of the float64 restatement; no bar is above 1e-4.  The select case is judged exactly."""
import ctypes
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

from pf3plat_amd import _lib
from tests import match_ref as ref

INVALID = -1
SCORES = ("matching_scores0", "matching_scores1", "scores")


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(ref.RECORDS))
def test_restatement_reproduces_the_reference_records(name):
    rec, B = ref.record(name), ref.RECORDS[name][0]
    for dtype in (torch.float64, torch.float32):
        r = ref.record_restatement(name, dtype)
        for key in ("matches0", "matches1"):
            assert torch.equal(r[key], rec[key]), (name, key, dtype)
        for key in ("matching_scores0", "matching_scores1"):
            err = ref.rel_l2(r[key], rec[key])
            print(name, key, dtype, err)
            assert r[key].shape == rec[key].shape and err < 2e-5, (name, key, err)
    assert int((rec["matches0"] > -1).sum()) >= 10 and len(r["matches"]) == B
    assert {n: s[:4] for n, s in ref.RECORDS.items()} == {"rec256": (2, 70, 150, 256), "rec64": (1, 45, 33, 64)}
    assert os.path.getsize(ref.FIXTURES) < 1 << 20


def test_cases_meet_their_conditions():
    sizes = {name: (c[1], c[2]) for name, c in ref.CASES.items()}
    assert sizes == {"n77": (((1, 77),), 32), "n1": (((40, 1),), 32), "e70": (((70, 150),), 32), "e131": (((131, 323),), 32),
                     "e323": (((323, 131),), 32), "e260": (((260, 517),), 32), "d1": (((70, 150),), 1), "d5": (((70, 150),), 5),
                     "d31": (((70, 150),), 31), "d64": (((70, 150),), 64), "d255": (((70, 150),), 255), "d256": (((70, 150),), 256),
                     "ragged": (((70, 150), (0, 33), (1, 77), (45, 0), (131, 323), (40, 1)), 32), "big": (((70, 150),), 32),
                     "z40": (((70, 150),), 32), "th0": (((70, 150),), 32), "th09": (((70, 150),), 32),
                     "select": (((256, 256), (256, 256)), 8)}
    assert (ref.CASES["th0"][4], ref.CASES["th09"][4]) == (0.0, 0.9) and all(c[4] == 0.1 for n, c in ref.CASES.items() if n not in ("th0", "th09"))
    assert ref.GAP == 100 * ref.MAX0_LOSS and ref.FLOOR <= ref.CAP
    for name in ref.CASES:
        gap, dist, big, loss = ref.conditions(name)
        print(name, "top-two gap", gap, "score to threshold", dist, "max |s|", big, "float32 loses on max0", loss)
        # the decisions are not within rounding: every row's and column's top-two gap of a and b, and every mutual score's distance
        # from the threshold.  Threshold 0 decides exp(max0) > 0, which only an underflow changes: there max0 stays far above -87.
        assert gap >= ref.GAP and dist >= ref.GAP, (name, gap, dist)
        assert loss <= ref.MAX0_LOSS * 1.5, (name, loss)
        r64, r32 = ref.restatement(name), ref.restatement(name, torch.float32)
        for a, b in zip(r64, r32):
            assert torch.equal(a["matches0"], b["matches0"]) and torch.equal(a["matches1"], b["matches1"]), name
        assert all(bar <= ref.CAP for bar in ref.bars(name).values()), name
    r = ref.restatement("th0")[0]
    mutual = r["matching_scores0"] > 0
    assert float(r["max0"][mutual].min()) > -40.0 and torch.equal(r["matches0"] > -1, mutual)
    assert ref.conditions("big")[2] >= 200.0  # exp overflows in float32 without the running maximum
    s = ref.case_of("big")["lists"][0]
    assert torch.isinf(torch.exp((s[0] @ s[1].T) / 32 ** 0.5)).any()
    # the threshold cuts through the mutual scores of a case, and the two other thresholds move the cut
    ms = ref.restatement("e70")[0]["matching_scores0"]
    assert 10 <= int((ms > 0.1).sum()) <= int((ms > 0).sum()) - 10
    for name, some in (("th0", False), ("th09", True)):  # threshold 0 keeps every mutual pair, 0.9 only a few
        r = ref.restatement(name)[0]
        kept, mutual = int((r["matches0"] > -1).sum()), int((r["matching_scores0"] > 0).sum())
        assert (1 <= kept < int((r["matching_scores0"] > 0.1).sum()) < mutual) if some else (kept == mutual >= 20), (name, kept, mutual)
    z = ref.case_of("z40")["lists"][0]
    assert set(z[2].abs().tolist()) == {40.0} and set(z[3].abs().tolist()) == {40.0} and (z[2] > 0).any() and (z[2] < 0).any()
    # the ragged case holds both kinds of empty list, and lists on either side of them
    found = [len(r["matches"]) for r in ref.restatement("ragged")]
    assert found[1] == found[3] == 0 and found[0] > 10 and found[4] > 10, found
    # select: 256 on the permutation, at most 192 elsewhere, integer operands, logits +-8
    case = ref.case_of("select")
    for l, (a0, a1, z0, z1) in enumerate(case["lists"]):
        perm = ref.select_permutation(ref.CASES["select"][0], l, 256)
        s = (a0.double() @ a1.double().T) * ref.SELECT_SCALE
        hot = torch.zeros_like(s).scatter_(1, perm[:, None], 1.0).bool()
        assert (s[hot] == 256.0).all() and float(s[~hot].max()) <= 192.0 and (a0 == a0.round()).all()
        assert set(z0.tolist()) == {8.0, -8.0} == set(z1.tolist())
        r = ref.restatement("select")[l]
        assert (r["matching_scores0"] > 0).all() and 0 < int((r["matches0"] > -1).sum()) < 256
    assert not torch.equal(ref.select_permutation(17, 0, 256), ref.select_permutation(17, 1, 256))


def test_floors_are_of_the_size_of_the_worst_float32_loss():
    loss = max(ref.conditions(n)[3] for n in ref.CASES)
    worst = max(ref.rel_l2(ref.scores_of(ref.restatement(n, torch.float32), k), ref.scores_of(ref.restatement(n), k)) for n in ref.CASES for k in SCORES)
    print("largest float32 loss of max0", loss, "MAX0_LOSS", ref.MAX0_LOSS, "; worst score loss", worst, "FLOOR", ref.FLOOR)
    # (the figures depend on the CPU's summation order: the order of magnitude is checked here, docs/PARITY.md section 21 has the
    # figures of the machine they were measured on)
    assert 0.5 * ref.MAX0_LOSS <= loss <= 1.5 * ref.MAX0_LOSS and 0.5 * ref.FLOOR <= worst <= 2.0 * ref.FLOOR


def test_symbols_are_declared_exported_and_listed():
    import pf3plat_amd
    from pf3plat_amd import matching

    for name in ("match_assignment", "pack_matched", "MatchAssignment", "Matches"):
        assert getattr(pf3plat_amd, name) is getattr(matching, name)
    lib = _lib.load()
    assert lib.gsr_abi_version() == 5 == _lib.GSR_ABI_VERSION
    exported = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    for name in ("gsr_match_assignment", "gsr_match_assignment_scratch_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(exported, name) and f"{name}(" in header, name
    assert len(lib.gsr_match_assignment_scratch_bytes.argtypes) == 4 and len(lib.gsr_match_assignment.argtypes) == 28
    assert lib.gsr_match_assignment_scratch_bytes.restype is ctypes.c_size_t
    with open(os.path.join(os.path.dirname(_lib.SRC), "gsr_attention.h")) as f:
        text = f.read()
    assert all(k in text for k in ("k_match_ops", "k_match_stream", "k_match_filter", "ma_mfma"))
    for name, (B, m, n, d, _) in ref.RECORDS.items():
        module = matching.MatchAssignment(d)
        state = ref.state_of(name)
        module.load_state_dict(state, strict=True)
        assert set(dict(module.named_parameters())) == set(state) == {"matchability.weight", "matchability.bias", "final_proj.weight", "final_proj.bias"}
        desc = ref.record_inputs(name)[0]
        assert torch.equal(module.get_matchability(desc), torch.sigmoid(desc @ state["matchability.weight"].T + state["matchability.bias"]).squeeze(-1))
    with pytest.raises(ValueError):
        matching.MatchAssignment(257)


def offsets(*lengths):
    out = [0]
    for n in lengths:
        out.append(out[-1] + n)
    return (ctypes.c_int32 * len(out))(*out)


def test_scratch_size_and_invalid_arguments_are_host_arithmetic():
    """Every call below returns before a launch: nothing is read through the device pointers, which are NULL."""
    lib = _lib.load()
    size = lib.gsr_match_assignment_scratch_bytes

    def call(L, d, off_m, off_n, scale=0.25, threshold=0.1, width=0, ptrs=None):
        ptrs = [None] * 20 if ptrs is None else ptrs  # mdesc0 .. z1 (4), the two device offsets, kpts0, kpts1, scratch, the 11 outputs
        return lib.gsr_match_assignment(L, d, scale, threshold, width, *ptrs[:4], off_m, ptrs[4], off_n, ptrs[5], *ptrs[6:], None)

    good = (offsets(70, 0, 5), offsets(150, 33, 0))
    assert size(3, *good, 32) == (75 + 183 + 1) * 16 and size(1, offsets(0), offsets(0), 1) == 16
    assert call(3, 32, *good) == INVALID  # good sizes, NULL required pointers
    bad = [(0, good, 32), (-1, good, 32), (3, good, 0), (3, good, 257), (3, good, -4),
           (3, (offsets(70, -1, 5), good[1]), 32), (3, (good[0], offsets(150, 33, -2)), 32), (2, ((ctypes.c_int32 * 3)(-1, 4, 8), good[1]), 32)]
    for L, (om, on), d in bad:
        assert size(L, om, on, d) == 0 and call(L, d, om, on) == INVALID, (L, d)
    assert size(3, None, good[1], 32) == 0 and size(3, good[0], None, 32) == 0 and call(3, 32, None, good[1]) == INVALID
    # every pointer set but one required pointer; then non-finite factors and keypoints without a width, with every pointer set
    fake = [ctypes.c_void_p(64)] * 20  # (never followed: each call below is refused before a launch)
    for scale, threshold in ((math.inf, 0.1), (-math.inf, 0.1), (math.nan, 0.1), (0.25, math.inf), (0.25, math.nan)):
        assert call(3, 32, *good, scale=scale, threshold=threshold, width=64, ptrs=fake) == INVALID
    assert call(3, 32, *good, width=0, ptrs=fake) == INVALID and call(3, 32, *good, width=-5, ptrs=fake) == INVALID
    one_kpts = list(fake)
    one_kpts[7] = None
    assert call(3, 32, *good, width=64, ptrs=one_kpts) == INVALID
    for missing in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15, 19):
        ptrs = list(fake)
        ptrs[missing] = None
        assert call(3, 32, *good, width=64, ptrs=ptrs) == INVALID, missing
    no_ids = list(fake)
    no_ids[16] = None
    assert call(3, 32, *good, width=64, ptrs=no_ids) == INVALID
    # a total times d at most 2^31 - 1, at its edge on either axis
    lim = 2 ** 31 - 1
    assert size(1, offsets(lim), offsets(5), 1) == (lim + 6) * 16 and size(1, offsets(5), offsets(lim), 1) == (lim + 6) * 16
    assert size(1, offsets(lim // 256), offsets(5), 256) > 0 and size(1, offsets(lim // 256 + 1), offsets(5), 256) == 0
    assert size(1, offsets(5), offsets(lim // 256), 256) > 0 and size(1, offsets(5), offsets(lim // 256 + 1), 256) == 0
    assert size(1, offsets(lim // 2 + 1), offsets(5), 2) == 0 and size(1, offsets(5), offsets(lim // 2 + 1), 2) == 0
    assert call(1, 2, offsets(lim // 2 + 1), offsets(5), ptrs=fake) == INVALID and call(1, 2, offsets(5), offsets(lim // 2 + 1), ptrs=fake) == INVALID


def test_python_checks_fire_in_order_and_refuse_cpu_tensors(monkeypatch):
    from pf3plat_amd import matching as mt

    def no_load():
        raise AssertionError("the library was loaded before the checks were through")

    monkeypatch.setattr(_lib, "load", no_load)
    a0, a1, z0, z1 = torch.zeros(2, 12, 8), torch.zeros(2, 20, 8), torch.zeros(2, 12, 1), torch.zeros(2, 20)
    bad = [((a0[0], a1, z0, z1), {}, "expected mdesc0"), ((a0, a1[:1], z0, z1), {}, "expected mdesc0"), ((a0, a1[..., :4], z0, z1), {}, "expected mdesc0"),
           ((a0, a1, z0[:, :5], z1), {}, "expected z0"), ((a0, a1, z0, z1[:, :5]), {}, "expected z1"), ((a0[:0], a1[:0], z0[:0], z1[:0]), {}, "at least one list"),
           ((torch.zeros(2, 12, 257), torch.zeros(2, 20, 257), z0, z1), {}, "d <= 256"), ((a0[..., :0], a1[..., :0], z0, z1), {}, "d <= 256"),
           ((a0, a1, z0, z1), {"lengths0": [12, 12]}, "go together"), ((a0[0], a1[0], z0[0], z1[0]), {"lengths0": [5, 7], "lengths1": [20]}, "as many"),
           ((a0[0], a1[0], z0[0], z1[0]), {"lengths0": [5, 6], "lengths1": [20, 0]}, "sum to 11"),
           ((a0[0], a1[0], z0[0], z1[0]), {"lengths0": [13, -1], "lengths1": [20, 0]}, ">= 0"),
           ((a0[0], a1[0], z0[0, :5], z1[0]), {"lengths0": [5, 7], "lengths1": [20, 0]}, "expected z0"),
           ((a0, a1, z0, z1), {"scale": float("inf")}, "finite"), ((a0, a1, z0, z1), {"threshold": float("nan")}, "finite"),
           ((a0, a1, z0, z1), {"kpts0": torch.zeros(2, 12, 2)}, "go together"),
           ((a0, a1, z0, z1), {"kpts0": torch.zeros(2, 12, 2), "kpts1": torch.zeros(2, 20, 2)}, "width"),
           ((a0, a1, z0, z1), {"kpts0": torch.zeros(2, 12, 2), "kpts1": torch.zeros(2, 20, 2), "width": 0}, "width"),
           ((a0, a1, z0, z1), {"kpts0": torch.zeros(2, 12, 2), "kpts1": torch.zeros(2, 19, 2), "width": 64}, "expected kpts1")]
    for args, kw, word in bad:  # CPU tensors all of them: the shapes are judged first
        with pytest.raises(ValueError, match=word):
            mt.match_assignment(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mt.match_assignment(a0, a1, z0, z1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mt.match_assignment(a0[0], a1[0], z0[0], z1[0], lengths0=[5, 7], lengths1=[20, 0], kpts0=torch.zeros(12, 2), kpts1=torch.zeros(20, 2), width=64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mt.MatchAssignment(8)(a0, a1)


def fake_matches(L):
    from pf3plat_amd.matching import Matches

    e = torch.zeros(0)
    ids = torch.zeros(0, dtype=torch.int64)
    return Matches(ids, ids, e, e, ids.int(), ids.int(), e, torch.zeros(L, dtype=torch.int32), (0,) * (L + 1), (0,) * (L + 1),
                                             ids, ids, torch.zeros(0, 2))


def test_pack_matched_refuses_a_list_count_that_is_not_scenes_times_pairs():
    from pf3plat_amd import pack_matched

    for L, scenes in ((5, 2), (4, 2), (7, 1), (6, 4), (3, 0), (8, 2)):
        with pytest.raises(ValueError, match="pairs"):
            pack_matched(fake_matches(L), scenes)
    for L, scenes, pairs in ((6, 2, 3), (1, 1, 1), (12, 4, 3), (12, 2, 6), (10, 1, 10)):
        packed, points = pack_matched(fake_matches(L), scenes)
        assert (packed.num_scenes, packed.num_pairs, packed.offsets) == (scenes, pairs, (0,) * (L + 1)) and tuple(points.shape) == (0, 2)
        assert tuple(packed.conf.shape) == (L,) and not packed.conf.any()
    with pytest.raises(ValueError, match="pixel ids"):
        pack_matched(fake_matches(6)._replace(ids_i=None), 2)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"
DENSE = ("matches0", "matches1", "matching_scores0", "matching_scores1")


def run_packed(name, **kw):
    from pf3plat_amd import match_assignment

    case = ref.case_of(name)
    a0, a1, z0, z1, len0, len1, k0, k1 = ref.packed(name)
    dev = lambda t: t.to(DEV)
    return match_assignment(dev(a0), dev(a1), dev(z0), dev(z1), len0, len1, threshold=case["threshold"], scale=case["scale"],
                            kpts0=dev(k0), kpts1=dev(k1), width=case["width"], **kw)


def to_host(got):
    keys = DENSE + ("idx0", "idx1", "scores", "counts", "ids_i", "ids_j", "points_2d")
    return got._replace(**{k: getattr(got, k).cpu() for k in keys if getattr(got, k) is not None})


@functools.lru_cache(maxsize=None)
def hip(name):
    """The HIP result of a case, computed once and shared."""
    return to_host(run_packed(name))


def expected_ids(kp, idx, width):
    p = kp[idx]
    return p[:, 1].long() * width + p[:, 0].long()  # the reference's `.long()`: truncation


@pytest.mark.gpu
@pytest.mark.parametrize("name", tuple(ref.CASES))
def test_hip_matches_the_float64_restatement(name):
    got, r64, case, bars = hip(name), ref.restatement(name), ref.case_of(name), ref.bars(name)
    off0, off1 = got.offsets0, got.offsets1
    assert len(off0) == len(r64) + 1 and got.matches0.dtype == torch.int64 and got.counts.dtype == torch.int32
    lists = got.lists()
    for l, r in enumerate(r64):  # list by list: every index exactly, every keypoint
        m0, m1 = got.matches0[off0[l]:off0[l + 1]], got.matches1[off1[l]:off1[l + 1]]
        assert torch.equal(m0, r["matches0"]) and torch.equal(m1, r["matches1"]), (name, l)
        k = len(r["matches"])
        assert int(got.counts[l]) == k, (name, l)
        assert torch.equal(lists[l][0].cpu(), r["matches"]) and lists[l][0].dtype == torch.int64, (name, l)
        kp0, kp1 = case["kpts"][l]
        sl = slice(off0[l], off0[l] + k)
        assert torch.equal(got.ids_i[sl], expected_ids(kp0, r["matches"][:, 0], case["width"])), (name, l)
        assert torch.equal(got.ids_j[sl], expected_ids(kp1, r["matches"][:, 1], case["width"])), (name, l)
        assert torch.equal(got.points_2d[sl], kp0[r["matches"][:, 0]]), (name, l)
    mine = {"matching_scores0": got.matching_scores0, "matching_scores1": got.matching_scores1, "scores": torch.cat([s.cpu() for _, s in lists])}
    for key in SCORES:
        want = ref.scores_of(r64, key)
        err = ref.rel_l2(mine[key], want)
        print(name, key, err, "bar", bars[key])
        assert mine[key].shape == want.shape and torch.isfinite(mine[key]).all() and err <= bars[key] <= ref.CAP, (name, key, err, bars[key])
    # a score is zero exactly where the restatement's is (no mutual partner), and nowhere else (nothing flushed)
    assert torch.equal(got.matching_scores0 > 0, ref.scores_of(r64, "matching_scores0") > 0)
    assert torch.equal(got.matching_scores1 > 0, ref.scores_of(r64, "matching_scores1") > 0)


@pytest.mark.gpu
def test_hip_ragged_lists_do_not_touch_one_another():
    """Each list of the ragged call alone, as a call of its own, gives the bits the list has inside the call; empty lists count 0."""
    from pf3plat_amd import match_assignment

    got, case = hip("ragged"), ref.case_of("ragged")
    assert got.counts.tolist()[1] == 0 and got.counts.tolist()[3] == 0
    assert (got.matches1[got.offsets1[1]:got.offsets1[2]] == -1).all() and not got.matching_scores1[got.offsets1[1]:got.offsets1[2]].any()
    assert (got.matches0[got.offsets0[3]:got.offsets0[4]] == -1).all() and not got.matching_scores0[got.offsets0[3]:got.offsets0[4]].any()
    for l in (0, 2, 4, 5):
        a0, a1, z0, z1 = (t.to(DEV) for t in case["lists"][l])
        one = to_host(match_assignment(a0[None], a1[None], z0[None], z1[None, :, None]))  # the equal-length form, B = 1
        m, n = a0.shape[0], a1.shape[0]
        assert tuple(one.matches0.shape) == (1, m) and tuple(one.matching_scores1.shape) == (1, n) and one.ids_i is None
        o0, o1, k = got.offsets0[l], got.offsets1[l], int(got.counts[l])
        assert int(one.counts[0]) == k
        assert torch.equal(one.matches0[0], got.matches0[o0:o0 + m]) and torch.equal(one.matches1[0], got.matches1[o1:o1 + n])
        assert torch.equal(one.matching_scores0[0], got.matching_scores0[o0:o0 + m]) and torch.equal(one.matching_scores1[0], got.matching_scores1[o1:o1 + n])
        for key in ("idx0", "idx1", "scores"):
            assert torch.equal(getattr(one, key)[:k], getattr(got, key)[o0:o0 + k]), (l, key)


@pytest.mark.gpu
def test_hip_select_is_exact():
    """s is 256 on a permutation and at most 192 elsewhere: m0 IS the permutation, both log-softmaxes are exactly 0 there, and the
    score is exp(ls(z0) + ls(z1[pi])).  Bound: the float32 sum carries the half-ulp errors of the two ls and of itself, each at most
    2^-24 of |sum| + 1, which exp turns into relative errors, and exp adds its own ulp."""
    got, case = hip("select"), ref.case_of("select")
    for l, (_, _, z0, z1) in enumerate(case["lists"]):
        perm = ref.select_permutation(ref.CASES["select"][0], l, 256)
        logs = F.logsigmoid(z0.double()) + F.logsigmoid(z1.double()[perm])
        want = logs.exp()
        sl = slice(got.offsets0[l], got.offsets0[l + 1])
        assert torch.equal(got.matches0[sl], torch.where(want > 0.1, perm, torch.full_like(perm, -1))), l
        rel = (got.matching_scores0[sl].double() / want - 1).abs()
        assert (rel <= 2.0 ** -23 * (2.0 + logs.abs())).all(), (l, float(rel.max()))
        assert torch.equal(got.matching_scores1[got.offsets1[l]:got.offsets1[l + 1]][perm], got.matching_scores0[sl]), l


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("e260", "ragged", "d255"))
def test_hip_repeats_bit_for_bit(name):
    first, again = hip(name), to_host(run_packed(name))
    counts = first.counts.tolist()
    assert torch.equal(first.counts, again.counts)
    for key in DENSE:
        assert torch.equal(getattr(first, key), getattr(again, key)), (name, key)
    for l, k in enumerate(counts):  # (entries past a list's count are not written)
        sl = slice(first.offsets0[l], first.offsets0[l] + k)
        for key in ("idx0", "idx1", "scores", "ids_i", "ids_j", "points_2d"):
            assert torch.equal(getattr(first, key)[sl], getattr(again, key)[sl]), (name, key, l)


@pytest.mark.gpu
@pytest.mark.parametrize("name", tuple(ref.RECORDS))
def test_hip_module_form_on_the_reference_records(name):
    from pf3plat_amd import MatchAssignment

    B, m, n, d, _ = ref.RECORDS[name]
    module = MatchAssignment(d)
    module.load_state_dict(ref.state_of(name), strict=True)
    desc0, desc1 = ref.record_inputs(name)
    got = to_host(module.to(DEV)(desc0.to(DEV), desc1.to(DEV)))
    rec, r64, r32 = ref.record(name), ref.record_restatement(name), ref.record_restatement(name, torch.float32)
    assert tuple(got.matches0.shape) == (B, m) and tuple(got.matches1.shape) == (B, n)
    assert torch.equal(got.matches0, rec["matches0"]) and torch.equal(got.matches1, rec["matches1"])
    for key in ("matching_scores0", "matching_scores1"):
        bar = max(ref.FLOOR, 4.0 * ref.rel_l2(r32[key], r64[key]))
        err, err_rec = ref.rel_l2(getattr(got, key), r64[key]), ref.rel_l2(getattr(got, key), rec[key])
        print(name, key, err, "bar", bar, "; against the record", err_rec)
        assert err <= bar <= ref.CAP and err_rec <= 2 * bar, (name, key, err, err_rec, bar)
    for b, (matches, scores) in enumerate(got.lists()):
        valid = rec["matches0"][b] > -1
        assert torch.equal(matches.cpu(), torch.stack([torch.where(valid)[0], rec["matches0"][b][valid]], -1))


@pytest.mark.gpu
def test_hip_pack_matched_feeds_the_coarse_poses():
    """A planted 2-scene, 3-view scene of the coarse-pose tests: `pack_matched` of the device assignment against `pose.pack_matches` of
    the restatement's lists - the same pack, and the same poses out of `coarse_poses`."""
    from pf3plat_amd import match_assignment, pack_matched, pose

    case = ref.pose_case("mixed")
    sc, width = case["scene"], case["width"]
    assert (sc.b, sc.v, len(case["lists"])) == (2, 3, 6)
    r64 = []
    for a0, a1, z0, z1 in case["lists"]:
        if a0.shape[0]:
            gap, _ = ref.gaps(a0, a1, z0, z1)
            assert gap >= ref.GAP
        r64.append({k: v[0] for k, v in ref.assignment(a0[None], a1[None], z0[None], z1[None]).items()})
    assert [len(r["matches"]) for r in r64] == [ls.ids_i.size for ls in sc.lists]  # every planted match is found
    cat = lambda k: torch.cat([ls[k] for ls in case["lists"]]).to(DEV)
    kcat = lambda k: torch.cat([kp[k] for kp in case["kpts"]]).to(DEV)
    got = match_assignment(cat(0), cat(1), cat(2), cat(3), [ls[0].shape[0] for ls in case["lists"]], [ls[1].shape[0] for ls in case["lists"]],
                           kpts0=kcat(0), kpts1=kcat(1), width=width)
    packed, points = pack_matched(got, sc.b)
    pairs = [(a, c) for a in range(sc.v) for c in range(a + 1, sc.v)]
    corr, pts = {p: [] for p in pairs}, []
    for l, (r, (kp0, kp1)) in enumerate(zip(r64, case["kpts"])):
        mt = r["matches"]
        corr[pairs[l // sc.b]].append((expected_ids(kp0, mt[:, 0], width).to(DEV), expected_ids(kp1, mt[:, 1], width).to(DEV), r["scores"].float().to(DEV)))
        pts.append(kp0[mt[:, 0]])
    want = pose.pack_matches(corr)
    assert packed.offsets == want.offsets and (packed.num_scenes, packed.num_pairs) == (want.num_scenes, want.num_pairs)
    assert torch.equal(packed.ids_i, want.ids_i) and torch.equal(packed.ids_j, want.ids_j) and torch.equal(packed.offsets_device, want.offsets_device)
    assert torch.equal(points.cpu(), torch.cat(pts)) and not packed.conf.any() and tuple(packed.conf.shape) == (6,)
    assert ref.rel_l2(packed.weights.cpu(), want.weights.cpu()) <= max(ref.FLOOR, 4.0 * ref.rel_l2(want.weights.cpu(), torch.cat([r["scores"] for r in r64])))
    # the 2-D points of ids_j are the scene's: ids_j is what the scene planted
    assert torch.equal(packed.ids_j.cpu(), torch.cat([torch.from_numpy(ls.ids_j)[r["matches"][:, 0]] for ls, r in zip(sc.lists, r64)]))
    xyz, K = torch.from_numpy(sc.xyz).to(DEV), torch.from_numpy(sc.intrinsics).to(DEV)
    mine = pose.coarse_poses(xyz, K, packed, points_2d=points)
    theirs = pose.coarse_poses(xyz, K, want, points_2d=torch.cat(pts).to(DEV))
    assert torch.equal(mine.pairwise, theirs.pairwise) and torch.equal(mine.inliers, theirs.inliers) and torch.equal(mine.status, theirs.status)
    assert int((mine.status == pose.STATUS_OK).sum()) >= 3
    assert torch.allclose(mine.confidence, theirs.confidence, rtol=1e-5, atol=0) and torch.allclose(mine.absolute, theirs.absolute, rtol=0, atol=1e-5)
