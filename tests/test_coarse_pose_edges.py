"""The coarse-pose chain where its first tests (tests/test_coarse_pose.py) could not reach: which hypothesis wins at the edges of the
blocks of 256, 4 and 8 views, fx != fy, the synchronisation at 5 - 8 views, the edges of the 1024-match LDS stage, ids outside the
image and non-finite points.

Yardsticks: tests/pnp_twin.py - the definition of include/gsr.h restated for the host around the shared solver - gives status, mask,
inlier count (compared EXACTLY) and pose for any (seed, hypotheses, list), the cases where a bad hypothesis is meant to win included;
tests/pnp_ref.py's float64 optimum over the planted inliers wherever the planted set is expected; the reference's own
`camera_synchronization` records for the synchronisation.  Every group has a test without a GPU that asserts that its inputs have
the property the group is about.  docs/PARITY.md section 16.1 records the measurements."""
import dataclasses
import functools
import hashlib

import numpy as np
import pytest
import torch

from pf3plat_amd import pose
from tests import pnp_ref as ref
from tests import pnp_twin
from tests.test_coarse_pose import FIXTURES, offsets_of, run

HW = ref.H * ref.W
FOCAL = (66.0, 54.0)  # fx != fy: a swap of k[0] and k[4] moves every projection
BLOCK = 256           # kPnpThreads: hypotheses per workgroup of k_pnp_hypotheses
# pairwise against the twin, in float32 ulps of the matrix's largest entry: 4 x the largest value measured on the MI355X over
# WINNER_CASES and the non-finite list (docs/PARITY.md section 16.1).  Measured: 0 in all 14 - every entry has the twin's bits.  Host
# and device run the same fp64 text without contraction and differ in libm alone (sqrt is exact in both; cos, acos, cbrt, sin are
# not), and an fp64 difference of an ulp or two almost never survives the rounding to float32.  4 x 0 is 0: a build whose libm moves
# one entry by one float32 ulp fails here and is to be measured again, not waved through.
TWIN_ULPS_MEASURED = 0.0
TWIN_ULPS = 4 * TWIN_ULPS_MEASURED
IDENTITY_BOUND = 1e-6  # |pairwise @ optimum - I|: about 10 x the float32 rounding of entries <= 1; an unrefined hypothesis: 1e-3
SEPARATION = 1e-3      # what two calls that must differ differ by, in some entry of `pairwise`


@pytest.fixture(scope="module", autouse=True)
def _built_twin(tmp_path_factory):
    pnp_twin.twin(tmp_path_factory)  # built once per session, under pytest's temporary directory


def twin():
    return pnp_twin.built()


def identity_error(pw, sc, ls):
    Ro, to = sc.optimum(ls)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Ro, to
    return np.abs(pw.astype(np.float64) @ T - np.eye(4)).max()


def check_against_twin(out, sc, l, e, label):
    """Status, inlier count and mask EXACTLY; the pose in ulps (printed before it is judged) -> the ulps."""
    ls = sc.lists[l]
    lo, hi = offsets_of(sc)[l], offsets_of(sc)[l + 1]
    pw = out["pairwise"][ls.scene, l // sc.b]
    u = ref.ulps(pw, e.pairwise.astype(np.float32))
    print(f"MEASURED {label}: status {out['status'][l]} inliers {out['inliers'][l]} (twin: {e.status}, {e.inliers}, winner t = {e.winner}, "
          f"score {e.score}), pairwise {u:.2f} ulps of the twin's")
    assert out["status"][l] == e.status and out["inliers"][l] == e.inliers, label
    assert np.array_equal(out["mask"][lo:hi].astype(bool), e.mask), label
    if e.status != pose.STATUS_OK:
        assert np.array_equal(pw, np.eye(4, dtype=np.float32)) and not out["mask"][lo:hi].any()
    else:
        assert np.isfinite(pw).all() and np.array_equal(pw[3], np.array([0, 0, 0, 1], dtype=np.float32))
    return u


# ---- a. which hypothesis wins -----------------------------------------------------------------------------------------------------
# One list of 60 matches: 10 exact inliers, 50 outliers >= 20 px away.  About one hypothesis in a thousand scores all ten inliers;
# the seeds below were found once by a search on the CPU (seeds 0 .. 11999 with the twin): T_STAR is the FIRST hypothesis that scores
# all ten.  With hypotheses = t* + 1 it is the very last one (low word 0) and must win; with hypotheses = t* the best of the earlier
# ones must, and refines to another pose.
@functools.lru_cache(maxsize=None)
def winner_scene():
    return ref.build_scene(21, 1, 2, ((60, 1 / 6, False),), focal=FOCAL)


T_STAR = {2061: 0, 4774: 255, 7859: 256, 5929: 511, 9877: 512, 10043: 1001, 5672: 1023}
REPEATED_DRAW_SEED = 11  # hypothesis 0 draws (2, 11, 11, 59): no triangle, no pose
# (seed, hypotheses); (2061, 1) is the call of one hypothesis with four distinct inliers, (5672, 1024) the last lane of four full blocks
WINNER_CASES = [(seed, t + 1) for seed, t in T_STAR.items()] + [(seed, t) for seed, t in T_STAR.items() if 0 < t < 1023] + [(REPEATED_DRAW_SEED, 1)]


@functools.lru_cache(maxsize=None)
def winner_expected(seed, hyp):
    return twin().expect(winner_scene(), 0, seed, hyp)


def test_winner_cases_exercise_what_they_claim():
    sc = winner_scene()
    ls = sc.lists[0]
    assert ls.ids_i.size == 60 and ls.inlier.sum() == 10 and sc.cam(ls)[0] != sc.cam(ls)[1]
    Ro, to = sc.optimum(ls)
    err = np.linalg.norm(ref.project(Ro, to, sc.cam(ls), sc.points(ls))[0] - ls.points_2d.astype(np.float64), axis=1)
    assert err[ls.inlier].max() <= 1e-4 and err[~ls.inlier].min() >= 19.9
    X, u, K = twin().fetch(sc, ls)
    assert sorted(T_STAR.values()) == [0, 255, 256, 511, 512, 1001, 1023]
    ties, blocks = 0, set()
    for seed, hyp in WINNER_CASES:
        e = winner_expected(seed, hyp)
        found, lo, hi = twin().hypotheses(X, u, K, seed, 0, hyp)
        print(f"seed {seed} hypotheses {hyp}: status {e.status}, winner t = {e.winner} (score {e.score}), {e.inliers} inliers, nearest error "
              f"to the threshold {e.margin:.3f} px (over all rounds {e.rounds_margin:.3f}), condition {e.condition:.2e}")
        assert e.decided, (seed, hyp)
        if seed == REPEATED_DRAW_SEED:
            d = twin().draws(60, seed, 0, 0)
            assert len(set(d[:3].tolist())) < 3 and not found[0] and e.status == pose.STATUS_NO_CONSENSUS and e.inliers == 0
            continue
        assert e.status == pose.STATUS_OK and e.margin >= 1e-3 and e.rounds_margin >= 1e-3 and e.condition <= 1e8, (seed, hyp)
        t = T_STAR[seed]
        if hyp == t + 1:
            # t* is the first hypothesis to score the ten planted inliers, it is the last of the call, and it refines to the planted set
            assert e.winner == t and e.score == 10 and (hi[:t] < 10).all() and np.array_equal(e.mask, ls.inlier)
            d = twin().draws(60, seed, 0, t)  # (three inliers give the planted pose among the P3P solutions; the fourth match chooses it)
            assert len(set(d[:3].tolist())) == 3 and ls.inlier[d[:3]].all() and (t > 0 or (len(set(d.tolist())) == 4 and ls.inlier[d].all()))
        else:
            other = winner_expected(seed, t + 1)
            assert e.winner < t and not np.array_equal(e.mask, ls.inlier)
            assert np.abs(e.pairwise - other.pairwise).max() >= SEPARATION or e.status != other.status, (seed, hyp)
            ties += int((hi[e.winner + 1:] == e.score).any())  # a later hypothesis ties with the winner: the lowest t must win
        blocks.add((e.winner // BLOCK, (hyp - 1) // BLOCK))
    assert ties >= 2
    # (the winner's block, the last block): the winner in the first, a middle and the last block of several - the maximum over the
    # blocks' slots decides - and the last hypothesis alone in its block (257, 513)
    assert {(0, 0), (0, 1), (1, 1), (1, 3), (2, 2), (3, 3)} <= blocks, blocks


def test_mutations_of_the_winner_search_change_an_expected_output():
    """What the kernels would return with a slip in the hypothesis indexing, worked out with the twin: each slip changes status, mask
    or pose (by >= SEPARATION) in at least one case, so the comparison with the twin sees it."""
    sc = winner_scene()
    ls = sc.lists[0]
    X, u, K = twin().fetch(sc, ls)

    def device_word_winner(found, lo, hyp, lanes):
        """The integer maximum of (score << 32) | uint32(hyp - 1 - t) over t < lanes."""
        t = np.arange(lanes, dtype=np.int64)
        words = np.where(found[:lanes] > 0, (lo[:lanes].astype(np.int64) << 32) | ((hyp - 1 - t) & 0xffffffff), 0)
        return words.max()

    def outcome(seed, t):
        st, count, mask, pw, *_ = twin().refine(X, u, K, seed, 0, t)
        return st, mask, pw

    def differs(a, b):
        return a[0] != b[0] or not np.array_equal(a[1], b[1]) or np.abs(a[2] - b[2]).max() >= SEPARATION

    seen = {"no guard": 0, "decode + 1": 0, "decode - 1": 0, "first slot only": 0, "last slot only": 0, "highest t of equals": 0, "fx and fy swapped": 0}
    for seed, hyp in WINNER_CASES:
        if seed == REPEATED_DRAW_SEED:
            continue
        e = winner_expected(seed, hyp)
        want = (e.status, e.mask, e.pairwise)
        lanes = -(-hyp // BLOCK) * BLOCK
        found, lo, hi = twin().hypotheses(X, u, K, seed, 0, lanes)
        assert np.array_equal(lo[:hyp], hi[:hyp]) or e.decided
        word = device_word_winner(found, lo, hyp, lanes)  # lanes past the end take part, with a huge low word
        seen["no guard"] += differs(outcome(seed, (hyp - 1 - int(word & 0xffffffff)) % (1 << 32) % lanes), want)
        for name, t in (("decode + 1", e.winner + 1), ("decode - 1", e.winner - 1)):
            if 0 <= t < hyp:
                seen[name] += differs(outcome(seed, t), want)
        for name, sl in (("first slot only", slice(0, BLOCK)), ("last slot only", slice(lanes - BLOCK, hyp))):
            f, s = found[sl], lo[sl]
            w = sl.start + int(np.argmax(np.where(f > 0, s, 0)))
            seen[name] += differs(outcome(seed, w), want)
        best = np.where(found[:hyp] > 0, lo[:hyp], 0)
        seen["highest t of equals"] += differs(outcome(seed, hyp - 1 - int(np.argmax(best[::-1]))), want)
        Ks = K[[1, 0, 2, 3]]
        w, _, _ = twin().winner(*twin().hypotheses(X, u, Ks, seed, 0, hyp))
        if w >= 0:
            st, count, mask, pw, *_ = twin().refine(X, u, Ks, seed, 0, w)
        seen["fx and fy swapped"] += w < 0 or differs((st, mask, pw), want)
    print({k: int(n) for k, n in seen.items()})
    assert all(n >= 1 for n in seen.values()), seen


@pytest.mark.gpu
@pytest.mark.parametrize("seed,hyp", WINNER_CASES)
def test_the_expected_hypothesis_wins_at_the_block_edges(seed, hyp):
    sc = winner_scene()
    ls = sc.lists[0]
    e = winner_expected(seed, hyp)
    out = run(sc, torch.device("cuda"), seed=seed, hypotheses=hyp)
    u = check_against_twin(out, sc, 0, e, f"winner seed {seed} hypotheses {hyp}")
    if seed != REPEATED_DRAW_SEED and hyp == T_STAR[seed] + 1:
        assert out["status"][0] == pose.STATUS_OK and np.array_equal(out["mask"].astype(bool), ls.inlier)
        err = identity_error(out["pairwise"][0, 0], sc, ls)
        print(f"MEASURED winner seed {seed} hypotheses {hyp}: |pairwise @ optimum - I| {err:.2e}")
        assert err <= IDENTITY_BOUND
    assert TWIN_ULPS is not None and u <= TWIN_ULPS, (u, TWIN_ULPS)


# ---- c. four and eight views, intrinsics per view ----------------------------------------------------------------------------------
def _view_focal(b, v):
    s, j = np.mgrid[0:b, 0:v]
    return np.stack([52.0 + 3.0 * j + 1.5 * s, 70.0 - 2.5 * j - 1.0 * s], -1)


def _view_specs(lists, empty, three):
    return tuple((0 if l == empty else 3 if l == three else 12 + (5 * l) % 13, 1.0, False) for l in range(lists))


VIEW_SCENES = {"v4_b2": (31, 2, 4, 5, 8), "v8_b1": (32, 1, 8, 9, 20)}  # name: (seed, b, v, the empty list, the list of three matches)


@functools.lru_cache(maxsize=None)
def view_scene(name):
    seed, b, v, empty, three = VIEW_SCENES[name]
    return ref.build_scene(seed, b, v, _view_specs(b * v * (v - 1) // 2, empty, three), focal=_view_focal(b, v))


def _inverse_of_optimum(sc, ls):
    Ro, to = sc.optimum(ls)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Ro.T, -Ro.T @ to
    return T


@pytest.mark.parametrize("name", list(VIEW_SCENES))
def test_view_scenes_exercise_what_they_claim(name):
    sc = view_scene(name)
    seed, b, v, empty, three = VIEW_SCENES[name]
    assert (sc.b, sc.v, len(sc.lists)) == (b, v, b * v * (v - 1) // 2) and len(sc.lists) == {"v4_b2": 12, "v8_b1": 28}[name]
    lengths = [ls.ids_i.size for ls in sc.lists]
    assert lengths[empty] == 0 and lengths[three] == 3 and all(12 <= n <= 24 for l, n in enumerate(lengths) if l not in (empty, three))
    k = sc.intrinsics.astype(np.float64)
    for s in range(b):  # every view's fx, fy, cx, cy differ from every other view's, and fx from fy
        for a in range(v):
            assert abs(k[s, a, 0, 0] - k[s, a, 1, 1]) >= 1.0
            for c in range(a + 1, v):
                assert abs(k[s, a, 0, 0] - k[s, c, 0, 0]) >= 1.0 and abs(k[s, a, 1, 1] - k[s, c, 1, 1]) >= 1.0
                assert k[s, a, 0, 2] != k[s, c, 0, 2] and k[s, a, 1, 2] != k[s, c, 1, 2]
    assert [ls.pair for ls in sc.lists[::b]] == ref.pairs_of(v) and [ls.scene for ls in sc.lists[:b]] == list(range(b))
    assert any(ls.pair[1] - ls.pair[0] > 1 for ls in sc.lists) and any(ls.pair[1] - ls.pair[0] == 1 for ls in sc.lists)
    planted = [l for l in range(len(sc.lists)) if l not in (empty, three)]
    inverses = {l: _inverse_of_optimum(sc, sc.lists[l]) for l in planted}
    for l in planted:
        ls = sc.lists[l]
        Ro, to = sc.optimum(ls)
        uv, z = ref.project(Ro, to, sc.cam(ls), sc.points(ls))
        assert ls.inlier.all() and np.linalg.norm(uv - ls.points_2d, axis=1).max() <= 1e-4 and (z > 0).all()
        for m in planted:  # every list has its own pose: a row in another list's place fails the identity check
            if m != l:
                assert np.abs(inverses[l] - inverses[m]).max() >= 10 * SEPARATION, (l, m)  # four orders above IDENTITY_BOUND
    conf = ref.expected_confidence(sc)
    far = np.array([ls.pair[1] - ls.pair[0] > 1 for ls in sc.lists])
    means = np.array([ls.scores.mean() if ls.scores.size else 0.0 for ls in sc.lists])
    assert (np.abs(conf[far & (means > 0)] - means[far & (means > 0)]) >= 1e-2).all()  # the relu'd value is not the mean: a wrong far flag shows


_VIEW_RESULTS = {}


def view_result(name):
    if name not in _VIEW_RESULTS:
        _VIEW_RESULTS[name] = run(view_scene(name), torch.device("cuda"))
    return _VIEW_RESULTS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VIEW_SCENES))
def test_every_pair_of_four_and_eight_views_gets_its_own_pose(name):
    sc, out = view_scene(name), view_result(name)
    seed, b, v, empty, three = VIEW_SCENES[name]
    off = offsets_of(sc)
    worst = 0.0
    for l, ls in enumerate(sc.lists):
        pw = out["pairwise"][ls.scene, l // b]
        if l in (empty, three):
            assert out["status"][l] == pose.STATUS_TOO_FEW_MATCHES and out["inliers"][l] == 0 and not out["mask"][off[l]:off[l + 1]].any()
            assert np.array_equal(pw, np.eye(4, dtype=np.float32))
            continue
        assert out["status"][l] == pose.STATUS_OK and out["inliers"][l] == ls.ids_i.size and out["mask"][off[l]:off[l + 1]].all(), l
        err = identity_error(pw, sc, ls)
        worst = max(worst, err)
        assert err <= IDENTITY_BOUND, (l, ls.pair, err)
    print(f"MEASURED {name}: |pairwise @ optimum - I| at most {worst:.2e} over {len(sc.lists) - 2} lists")
    want = ref.expected_confidence(sc)
    assert np.abs(out["confidence"] - want).max() <= 4 * np.finfo(np.float32).eps, (out["confidence"], want)
    assert out["confidence"][empty] == 0
    dev = torch.device("cuda")
    absolute = pose.synchronize_cameras(torch.from_numpy(out["pairwise"]).to(dev), torch.from_numpy(out["confidence"]).to(dev), v)
    assert np.array_equal(absolute.cpu().numpy(), out["absolute"]) and np.isfinite(out["absolute"]).all()


# ---- d. the synchronisation at 5, 6 and 8 views -------------------------------------------------------------------------------------
# sha256 (first 16 hex digits) of every array the fixture file held before v5_b2 .. zero_v5 were appended
OLD_RECORDS = {
    "far_low/absolute": "11d2d941d54f1b94", "far_low/confidence": "2103e8ea2024d15e", "far_low/means": "9d1fc237e00d1ae4",
    "far_low/pairwise": "8be2d81fa01a3ba3", "far_low/views": "35be322d094f9d15",
    "v2_b1/absolute": "ada4af2684f266e6", "v2_b1/confidence": "8ddfdf80a56d9235", "v2_b1/means": "8ddfdf80a56d9235",
    "v2_b1/pairwise": "2a83daf69a457e05", "v2_b1/views": "d86e8112f3c4c444",
    "v2_b2/absolute": "2a2c8453cc479550", "v2_b2/confidence": "ad606540ad8d1ace", "v2_b2/means": "ad606540ad8d1ace",
    "v2_b2/pairwise": "5f5db308a274a547", "v2_b2/views": "d86e8112f3c4c444",
    "v3_b1/absolute": "f18804b8fd675668", "v3_b1/confidence": "2ee31108201ad8aa", "v3_b1/means": "af75e385650e4947",
    "v3_b1/pairwise": "540458f5690ef0cc", "v3_b1/views": "35be322d094f9d15",
    "v3_b2/absolute": "fa86297b6eb43120", "v3_b2/confidence": "3694255268d97e5a", "v3_b2/means": "ca7e8ec11b805245",
    "v3_b2/pairwise": "7158c4ec04bdfdf5", "v3_b2/views": "35be322d094f9d15",
    "v4_b1/absolute": "417805d6aa990a18", "v4_b1/confidence": "39c53ae9aa34b91f", "v4_b1/means": "6b1a7fe8db91cb41",
    "v4_b1/pairwise": "365f0aace6c9ff44", "v4_b1/views": "f0a0278e4372459c",
    "v4_b2/absolute": "d23403256e43be5b", "v4_b2/confidence": "604b0e7d07887f39", "v4_b2/means": "97c5d1df40bfe4dc",
    "v4_b2/pairwise": "3a8ab4ea4c30e2b0", "v4_b2/views": "f0a0278e4372459c",
    "zero/absolute": "99ad000dcb5a918d", "zero/confidence": "15ec7bf0b50732b4", "zero/means": "15ec7bf0b50732b4",
    "zero/pairwise": "326423b8c723fbaf", "zero/views": "35be322d094f9d15",
}
NEW_RECORDS = {"v5_b2": (5, 2), "v6_b1": (6, 1), "v8_b1": (8, 1), "v8_b2": (8, 2), "zero_v5": (5, 1)}


def test_sync_records_keep_the_old_arrays_and_add_the_large_ones():
    with np.load(FIXTURES) as fx:
        for key, digest in OLD_RECORDS.items():
            assert hashlib.sha256(np.ascontiguousarray(fx[key]).tobytes()).hexdigest()[:16] == digest, key
        names = [str(n) for n in fx["names"]]
        assert names[:8] == ["v2_b1", "v2_b2", "v3_b1", "v3_b2", "v4_b1", "v4_b2", "far_low", "zero"] and names[8:] == list(NEW_RECORDS)
        for name, (v, b) in NEW_RECORDS.items():
            pairs = v * (v - 1) // 2
            assert int(fx[name + "/views"]) == v and fx[name + "/pairwise"].shape == (b, pairs, 4, 4) and fx[name + "/confidence"].shape == (pairs * b,)
            assert fx[name + "/absolute"].shape == (b, v, 4, 4) and fx[name + "/absolute"].dtype == np.float32
            assert 16 * v * v > 256 or v < 5  # the squaring loop takes more than one trip per lane
            if name != "zero_v5":  # far pairs of every span carry the relu'd confidence, neighbours the mean score
                far = np.repeat([c - a > 1 for a, c in ref.pairs_of(v)], b)
                conf, means = fx[name + "/confidence"], fx[name + "/means"]
                assert np.array_equal(conf[~far], means[~far]) and (conf[far] < means[far] - 0.04).all() and (conf > 0).all()
        assert (fx["zero_v5/confidence"] == 0).all()
        chained = ref.camera_chaining(fx["zero_v5/pairwise"][0], 5)
        assert np.array_equal(chained, fx["zero_v5/absolute"][0])  # the record is of the fallback: pairs (0,1) (1,2) (2,3) (3,4) = rows 0, 4, 7, 9
        assert [ref.pairs_of(5).index((i, i + 1)) for i in range(4)] == [0, 4, 7, 9]


@pytest.mark.gpu
def test_synchronisation_of_five_to_eight_views_agrees_with_the_reference_records():
    dev = torch.device("cuda")
    with np.load(FIXTURES) as fx:
        rec = {k: fx[k] for k in fx.files}
    for name, (v, b) in NEW_RECORDS.items():
        got = pose.synchronize_cameras(torch.from_numpy(rec[name + "/pairwise"]).to(dev), torch.from_numpy(rec[name + "/confidence"]).to(dev), v)
        u = ref.ulps(got.cpu().numpy(), rec[name + "/absolute"])
        print(f"MEASURED sync {name}: {u:.2f} ulps")
        assert u <= 4, (name, u)
    # the five-view fallback scene batched with the first scene of v5_b2: each as a scene of its own (the decision is per scene)
    Ps = np.concatenate([rec["v5_b2/pairwise"][:1], rec["zero_v5/pairwise"]])
    conf = np.stack([rec["v5_b2/confidence"][0::2], rec["zero_v5/confidence"]], 1).reshape(-1)  # list order: pair-major
    got = pose.synchronize_cameras(torch.from_numpy(Ps).to(dev), torch.from_numpy(conf).to(dev), 5).cpu().numpy()
    alone = pose.synchronize_cameras(torch.from_numpy(Ps[:1]).to(dev), torch.from_numpy(rec["v5_b2/confidence"][0::2].copy()).to(dev), 5).cpu().numpy()
    assert np.array_equal(got[:1], alone) and ref.ulps(got[:1], rec["v5_b2/absolute"][:1]) <= 4
    assert ref.ulps(got[1:], rec["zero_v5/absolute"]) <= 4 and np.array_equal(got[1, 0], np.eye(4, dtype=np.float32))


# ---- e. the edges of the LDS stage (kPnpStage = 1024) --------------------------------------------------------------------------------
STAGE_LENGTHS = (1023, 1024, 1025, 2049)  # a stage one short of full, a full stage with no tail, a tail of one, three stages


@functools.lru_cache(maxsize=None)
def stage_scene():
    return ref.build_scene(41, 4, 2, tuple((n, 0.4, True) for n in STAGE_LENGTHS), focal=FOCAL)


@pytest.mark.parametrize("l", range(len(STAGE_LENGTHS)))
def test_stage_lists_exercise_what_they_claim(l):
    sc = stage_scene()
    ls = sc.lists[l]
    assert ls.ids_i.size == STAGE_LENGTHS[l] and ls.inlier.sum() == int(np.ceil(0.4 * STAGE_LENGTHS[l]))
    Ro, to = sc.optimum(ls)
    uv, z = ref.project(Ro, to, sc.cam(ls), sc.points(ls))
    err = np.linalg.norm(uv - ls.points_2d.astype(np.float64), axis=1)
    print(f"stage[{l}] n={err.size}: inliers within {err[ls.inlier].max():.3f} px, outliers beyond {err[~ls.inlier].min():.3f} px")
    assert err[ls.inlier].max() <= 2.5 and err[~ls.inlier].min() >= 10.0 and (z > 0).all()
    assert ls.ids_j.min() >= 0 and ls.ids_j.max() < HW and ls.ids_i.min() >= 0 and ls.ids_i.max() < HW
    # the last match of a stage and the first of the next are one of each kind somewhere: a dropped or doubled match shows in the mask
    assert ls.inlier[1000:].any() and (~ls.inlier[1000:]).any()


_STAGE_RESULT = {}


@pytest.mark.gpu
@pytest.mark.parametrize("l", range(len(STAGE_LENGTHS)))
def test_consensus_set_at_the_stage_edges_equals_the_planted_one(l):
    sc = stage_scene()
    if "out" not in _STAGE_RESULT:
        _STAGE_RESULT["out"] = run(sc, torch.device("cuda"))
    out, ls = _STAGE_RESULT["out"], sc.lists[l]
    lo, hi = offsets_of(sc)[l], offsets_of(sc)[l + 1]
    assert out["status"][l] == pose.STATUS_OK and out["inliers"][l] == ls.inlier.sum()
    assert np.array_equal(out["mask"][lo:hi].astype(bool), ls.inlier)  # EQUAL
    err = identity_error(out["pairwise"][ls.scene, 0], sc, ls)
    print(f"MEASURED stage n={STAGE_LENGTHS[l]}: |pairwise @ optimum - I| {err:.2e}")
    assert err <= IDENTITY_BOUND


# ---- f. ids outside the image, non-finite points ------------------------------------------------------------------------------------
OUTSIDE = (-1, -2 ** 40, HW, 2 ** 40)
CLAMPED = (0, 0, HW - 1, HW - 1)
NON_FINITE = ((np.nan, np.nan, np.nan), (0.3, -0.2, np.inf), (-np.inf, 0.1, 2.0), (0.5, np.nan, 3.0), (np.inf, np.inf, np.inf))


@functools.lru_cache(maxsize=None)
def abuse_scenes():
    """-> (the scene with list 0's four ids written outside the image, the same with them written clamped, the matches changed in
    list 0, those in list 1).  In both, five outliers of list 1 (scene 1) have non-finite 3-D points."""
    base = ref.build_scene(51, 2, 2, ((64, 0.5, True), (65, 0.5, True)), focal=FOCAL)
    xyz = base.xyz.copy()
    k0 = np.flatnonzero(~base.lists[0].inlier)[2:6]  # (the first two outliers hold the corner ids)
    k1 = np.flatnonzero(~base.lists[1].inlier)[2:7]
    flat = xyz[1, 1].reshape(3, -1)
    for k, value in zip(k1, NON_FINITE):
        flat[:, base.lists[1].ids_j[k]] = value
    scenes = []
    for ids in (OUTSIDE, CLAMPED):
        ids_j = base.lists[0].ids_j.copy()
        ids_j[k0] = ids
        scenes.append(dataclasses.replace(base, xyz=xyz, lists=[dataclasses.replace(base.lists[0], ids_j=ids_j), base.lists[1]]))
    return scenes[0], scenes[1], k0, k1


def test_abuse_lists_exercise_what_they_claim():
    outside, clamped, k0, k1 = abuse_scenes()
    a, c = outside.lists[0], clamped.lists[0]
    assert a.ids_j[k0].tolist() == list(OUTSIDE) and c.ids_j[k0].tolist() == list(CLAMPED) and not a.inlier[k0].any()
    rest = np.setdiff1d(np.arange(64), k0)
    assert np.array_equal(a.ids_j[rest], c.ids_j[rest]) and c.ids_j.min() >= 0 and c.ids_j.max() < HW
    X, u, K = twin().fetch(outside, a)
    Xc, _, _ = twin().fetch(clamped, c)
    assert np.array_equal(X, Xc) and np.isfinite(X).all()  # the twin clamps as the definition promises
    e = twin().expect(clamped, 0, 0, 1000)
    assert e.status == pose.STATUS_OK and np.array_equal(e.mask, c.inlier) and e.margin >= 1e-3  # the four stay outliers at the clamped pixels
    ls = outside.lists[1]
    X, u, K = twin().fetch(outside, ls)
    bad = ~np.isfinite(X).all(1)
    assert np.array_equal(np.flatnonzero(bad), k1) and not ls.inlier[k1].any()  # the five pixels are no other match's
    assert np.isnan(X[k1]).any() and (X[k1] == np.inf).any() and (X[k1] == -np.inf).any()
    e = twin().expect(outside, 1, 0, 1000)
    assert e.status == pose.STATUS_OK and np.array_equal(e.mask, ls.inlier) and not e.mask[k1].any() and e.margin >= 1e-3
    assert np.isfinite(e.pairwise).all() and e.condition <= 1e8
    found, lo, hi = twin().hypotheses(X, u, K, 0, 1, 1000)
    drew_bad = np.array([bad[twin().draws(65, 0, 1, t)].any() for t in range(1000)])
    assert drew_bad.sum() >= 100 and not found[drew_bad].any()  # many hypotheses draw a non-finite point: none of them has a pose


@pytest.mark.gpu
def test_ids_outside_the_image_are_clamped_and_non_finite_points_fail_every_test():
    outside, clamped, k0, k1 = abuse_scenes()
    dev = torch.device("cuda")
    got, want = run(outside, dev), run(clamped, dev)
    for k in got:
        assert np.array_equal(got[k], want[k], equal_nan=True), k  # bit-equal to the same call with the ids written clamped
    assert np.array_equal(got["mask"][:64].astype(bool), outside.lists[0].inlier) and got["status"][0] == pose.STATUS_OK
    e = twin().expect(outside, 1, 0, 1000)
    u = check_against_twin(got, outside, 1, e, "non-finite points")
    ls = outside.lists[1]
    assert got["status"][1] == pose.STATUS_OK and np.array_equal(got["mask"][64:].astype(bool), ls.inlier) and not got["mask"][64:][k1].any()
    assert np.isfinite(got["pairwise"]).all() and np.isfinite(got["absolute"]).all()
    assert TWIN_ULPS is not None and u <= TWIN_ULPS, (u, TWIN_ULPS)
