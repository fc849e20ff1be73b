"""Keypoint extraction on the device (pf3plat_amd.keypoints; gsr_keypoints; definition: include/gsr.h) against tests/keypoint_ref.py -
the reference's lines restated, float64 the yardstick - and against the records of the reference's own simple_nms, top_k_keypoints
and sample_descriptors, tests/golden/keypoint_fixtures.npz.

Bars (docs/PARITY.md section 22, conventions of section 21): in the scores form pixels, counts and order EQUAL the restatement on
every case, ties included; in the logits form the same, on cases whose decisions keep GAP away from rounding (asserted on the CPU);
keypoint scores and descriptors within max(FLOOR, 4 x |float32 restatement - float64 restatement|) rel-L2 of the float64
restatement and never above 1e-4; rescaled keypoints within 2^-22 (pixel + 0.5) / scale of float64.

Measured on one MI355X: every pixel, count and order equal on every case; keypoint scores within 4.0e-7 (bars 4.1e-7 to 1.6e-6),
descriptors within 6.5e-7 (bars 6.6e-7 to 2.6e-6), at most 0.26 of a bar; rescaled keypoints within 0.23 of their bound.

The loops only large calls enter (docs/PARITY.md section 22.1): the scan past 2048 mask words, the packed base of an image past
256, the top-k rank count past 8192 staged keypoints - scores form, exact; the CPU test states what each case reaches."""
import ctypes
import functools
import os

import pytest
import torch

from pf3plat_amd import _lib
from tests import keypoint_ref as ref

F64, F32 = torch.float64, torch.float32
cat = lambda results, key: torch.cat([r[key] for r in results])


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (F64, F32))
def test_restatement_reproduces_the_reference_records(dtype):
    for name, (_, B, H, W, _, r) in ref.SCORE_CASES.items():
        s = ref.score_case(name).to(dtype)
        assert torch.equal(ref.nms_mask(s, r) & (s > 0), ref.unpack_mask("nms." + name, (B, H, W))), name
    for direction in "hvd":
        s, want = ref.staircase(direction)
        kept = ref.nms_mask(s.to(dtype), 4) & (s > 0)
        assert torch.equal(kept, ref.unpack_mask("stairs." + direction, tuple(s.shape))), direction
        got = ref.select(s.to(dtype), remove_borders=0)
        assert [[tuple(p) for p in pix.tolist()] for pix, _, _ in got] == [sorted(w, key=lambda p: (p[1], p[0])) for w in want]
    assert ref.fixtures()["stairs.seven"].tolist() == [3, 11, 19]  # of seven stairs from x = 3: 0, 2, 4 - never the seventh
    pix, desc = ref.sample_inputs()
    err = ref.rel_l2(ref.sample(pix, desc[0], dtype), torch.from_numpy(ref.fixtures()["sample"]))
    print(f"sample_descriptors record, {dtype}: rel-L2 {err:.3e}")
    assert err <= 2e-5
    scores, k = ref.topk_inputs()
    assert torch.equal(torch.sort(scores.to(dtype), descending=True, stable=True).indices[:k], torch.from_numpy(ref.fixtures()["topk"]))


def test_cases_meet_their_conditions():
    from pf3plat_amd import keypoints

    assert keypoints.TILE == ref.TILE and ref.TILE % 8 == 0
    sizes = {(8 * c[2], 8 * c[3]) for c in ref.LOGIT_CASES.values()}
    T = ref.TILE
    assert {(8, 8), (16, 24), (24, 24), (72, 136), (T - 8, T), (T, T + 8), (2 * T + 8, T - 8), (T + 8, 2 * T + 8), (128, 128)} <= sizes
    worst = 0.0
    for name, case in ref.LOGIT_CASES.items():
        gap, near, found = ref.conditions(name)
        loss = ref.score_loss(name)
        worst = max(worst, loss)
        print(f"{name}: window gap {gap:.3e}, candidate to threshold {near:.3e}, found {found}, score loss {loss:.3e}")
        assert gap >= ref.GAP and near >= ref.GAP, name
        r64, r32 = ref.logit_reference(name)
        for a, b in zip(r64, r32):  # float32 decides as float64 does: the cases are fair
            assert torch.equal(a["pixels"], b["pixels"]) and a["count"] == b["count"]
    assert ref.SCORE_LOSS / 10 <= worst <= ref.SCORE_LOSS * 1.5 and ref.GAP <= ref.CAP * 2
    counts = lambda name: [r["count"] for r in ref.logit_reference(name)[0]]
    assert counts("s1x1") == [0]
    b = counts("batch")
    assert b[1] == 0 and b[0] != b[2] and min(b[0], b[2]) > 100
    for name in ("w2p8", "topk"):  # the planted ties survive: equal scores among the keypoints of an image
        for r in ref.logit_reference(name)[0]:
            s = r["keypoint_scores"]
            assert s.numel() - s.unique().numel() >= 3, name
    # the top-k cut orders scores of distant pixels: the two it cuts between, and every two of its order, differ by GAP or are planted ties
    for r in ref.logit_reference("topk")[0]:
        s = r["keypoint_scores"].unique()
        assert float(((s[1:] - s[:-1]) / s[1:]).min()) >= ref.GAP
    # remove_borders 0 reaches the zero padding of the sampling at the image corner
    pix = cat(ref.logit_reference("b0")[0], "pixels")
    assert int((pix.min(1).values < 3).sum()) > 0


def test_floors_are_of_the_size_of_the_worst_float32_loss():
    worst_s = worst_d = 0.0
    for name in ref.LOGIT_CASES:
        r64, r32 = ref.logit_reference(name)
        if sum(r["count"] for r in r64):
            worst_s = max(worst_s, ref.rel_l2(cat(r32, "keypoint_scores"), cat(r64, "keypoint_scores")))
            worst_d = max(worst_d, ref.rel_l2(cat(r32, "descriptors"), cat(r64, "descriptors")))
    print(f"float32 restatement: scores {worst_s:.3e}, descriptors {worst_d:.3e}")
    assert ref.FLOOR_SCORES / 10 <= worst_s <= ref.FLOOR_SCORES * 1.5 and ref.FLOOR_DESCRIPTORS / 10 <= worst_d <= ref.FLOOR_DESCRIPTORS * 1.5
    assert max(ref.FLOOR_SCORES, ref.FLOOR_DESCRIPTORS) * 4 <= ref.CAP


def test_large_cases_take_the_scan_the_base_and_the_top_k_past_their_first_trip():
    """The three loops of gsr_attention.h's keypoint passes that only large calls enter, each with what it carries.
    k_keypoint_scan: 2048 mask words a trip, `running` the keypoints counted so far - keypoints lie on both sides of word 2048, so
    a lost count moves the later ones onto the first rows.  kp_base: the counts of the images before b, 256 a trip - image 256 is not
    empty, so the rows of 257 ... 259 start past a second trip's sum, in the write, the top-k and the descriptor pass.
    k_keypoint_topk: 8192 staged keypoints a trip, every keypoint's rank so far reloaded - equal scores lie on both sides of every
    chunk edge, and the ranks without any one chunk's share keep another set."""
    from pf3plat_amd import keypoints

    with open(os.path.join(os.path.dirname(_lib.SRC), "gsr_attention.h")) as f:
        text = f.read()
    for line in (f"base += {ref.SCAN_CHUNK})", f"i += {ref.BASE_STEP}) mine +=", f"kKpTopkChunk = {ref.TOPK_CHUNK};"):
        assert line in text, line  # the trip lengths the cases are sized by are the source's
    # the scan
    words = {}
    for name, (_, H, W, r, border) in ref.SCAN_CASES.items():
        s, _, want = ref.scan_case(name)
        pix, sc, n = want[0]
        w = ref.mask_words(pix, W)
        words[name] = H * (-(-W // keypoints.TILE))
        first = int((w < ref.SCAN_CHUNK).sum())
        print(f"scan {name}: {words[name]} words, {n} keypoints, {n - first} of them in words from {ref.SCAN_CHUNK} on")
        assert n == first + int((w >= ref.SCAN_CHUNK).sum()) and first > 0
        assert (n - first > 0) == (words[name] > ref.SCAN_CHUNK)
        assert sc.numel() - sc.unique().numel() > n // 2  # eighths: ties
    assert words == {"w2048": ref.SCAN_CHUNK, "w2049": ref.SCAN_CHUNK + 1, "w2080": ref.SCAN_CHUNK + 32}
    # the batch
    _, B, H, W, r, border, thr, k, C = ref.BATCH_CASE
    s, desc, kw = ref.batch_case()
    counts = [n for _, _, n in ref.select(s, **kw)]
    print(f"batch: {B} images, counts 0 .. {max(counts)}, {counts.count(0)} empty, {sum(n > k for n in counts)} above the cut of {k}; the last: {counts[250:]}")
    assert B > ref.BASE_STEP + 1 and tuple(s.shape) == (B, 8, 8) and tuple(desc.shape) == (B, 8, 1, 1)
    assert counts[0] > 0 and counts[ref.BASE_STEP] > 0 and counts.count(0) > 0 and len(set(counts)) > 3
    assert all(counts[b] > k for b in range(ref.BASE_STEP + 1, B))  # the images whose base takes a second trip are staged by the cut
    assert any(0 < n <= k for n in counts) and any(n > k for n in counts[:ref.BASE_STEP])
    # the top-k
    trips = {}
    for name, (_, H, W, found, k) in ref.TOPK_CASES.items():
        s, kw, want, staged = ref.topk_case(name)
        n = want[0][2]
        trips[name] = -(-n // ref.TOPK_CHUNK)
        assert n == staged.numel() == (found or n) and n / 2 < k < n <= H * W and len(want[0][1]) == k and staged.unique().numel() == 8
        shares = ref.chunk_ranks(staged)
        rank = shares.sum(0)
        order = torch.sort(staged, descending=True, stable=True).indices
        assert torch.equal(rank[order], torch.arange(n)) and shares.shape[0] == trips[name]
        print(f"top-k {name}: {n} found, {k} kept, {trips[name]} chunks")
        for c in range(trips[name] if trips[name] > 1 else 0):  # without chunk c's share of the ranks another set is kept
            assert not torch.equal(rank - shares[c] < k, rank < k), (name, c)
        for edge in range(ref.TOPK_CHUNK, n, ref.TOPK_CHUNK):  # equal scores on both sides of the edge, the earlier one kept
            lo, after = torch.arange(n) < edge, staged[edge:edge + ref.TOPK_CHUNK]
            assert bool((lo & (rank < k) & torch.isin(staged, after)).any()), (name, edge)
            assert bool((rank[edge:edge + ref.TOPK_CHUNK] < k).any())  # ... and one past the edge is kept: its rank counts the earlier equal ones
    assert trips == {"k8192": 1, "k8193": 2, "k3trips": 3}
    assert ref.TOPK_CASES["k8192"][3] == ref.TOPK_CHUNK and ref.TOPK_CASES["k8193"][3] == ref.TOPK_CHUNK + 1


REFERENCE_CONVS = {"conv1a": (64, 1, 3), "conv1b": (64, 64, 3), "conv2a": (64, 64, 3), "conv2b": (64, 64, 3), "conv3a": (128, 64, 3),
                   "conv3b": (128, 128, 3), "conv4a": (128, 128, 3), "conv4b": (128, 128, 3), "convPa": (256, 128, 3), "convPb": (65, 256, 1),
                   "convDa": (256, 128, 3), "convDb": (256, 256, 1)}


def reference_state(seed=5):
    """A state dict with the reference's key set and shapes (superpoint.py:127-142), seeded."""
    g, state = ref.gen(seed), {}
    for name, (o, i, k) in REFERENCE_CONVS.items():
        state[name + ".weight"] = torch.randn(o, i, k, k, generator=g) * (2.0 / (i * k * k)) ** 0.5
        state[name + ".bias"] = 0.1 * torch.randn(o, generator=g)
    return state


def test_symbols_are_declared_exported_and_listed():
    import pf3plat_amd
    from pf3plat_amd import keypoints

    for name in ("detect_keypoints", "keypoints_from_scores", "Keypoints", "SuperPoint"):
        assert getattr(pf3plat_amd, name) is getattr(keypoints, name)
    lib = _lib.load()
    assert lib.gsr_abi_version() == 5 == _lib.GSR_ABI_VERSION and lib.gsr_keypoints_tile() == keypoints.TILE
    exported = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    for name in ("gsr_keypoints", "gsr_keypoints_scratch_bytes", "gsr_keypoints_tile"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(exported, name) and f"{name}(" in header, name
    assert len(lib.gsr_keypoints_scratch_bytes.argtypes) == 5 and len(lib.gsr_keypoints.argtypes) == 22
    assert lib.gsr_keypoints_scratch_bytes.restype is ctypes.c_size_t
    with open(os.path.join(os.path.dirname(_lib.SRC), "gsr_attention.h")) as f:
        text = f.read()
    assert all(k in text for k in ("k_keypoint_ops", "k_keypoint_scores", "k_keypoint_nms", "k_keypoint_scan", "k_keypoint_write",
                                   "k_keypoint_topk", "k_keypoint_desc"))
    module = keypoints.SuperPoint()
    module.load_state_dict(reference_state(), strict=True)
    assert set(module.state_dict()) == {f"{n}.{p}" for n in REFERENCE_CONVS for p in ("weight", "bias")}


def test_scratch_size_and_invalid_arguments_are_host_arithmetic():
    """Every call below returns before a launch: nothing is read through the device pointers."""
    lib = _lib.load()
    size = lib.gsr_keypoints_scratch_bytes
    assert size(3, 37, 61, 0, 100) == 3 * (2 * 37 * 2 + 3 * 100) * 4 and size(1, 8, 8, 256, 1) == (2 * 8 + 3) * 4
    for args in ((0, 8, 8, 8, 4), (65536, 8, 8, 8, 4), (1, 0, 8, 8, 4), (1, 8, 8, 257, 4), (1, 8, 8, -1, 4), (1, 8, 8, 8, 0), (1, 12, 8, 8, 4),
                 (1, 8, 12, 8, 4), (2, 32768, 32768, 0, 4), (2, 8, 8, 256, 2 ** 22)):
        assert size(*args) == 0, args
    fake = ctypes.c_void_p(64)  # (never followed)
    strides = (ctypes.c_int64 * 4)(512, 64, 8, 1)

    def call(mode=0, B=1, H=8, W=8, C=8, r=4, thr=0.0005, border=4, k=0, cap=4, logits=fake, scores=fake, desc=fake, st=strides, work=fake,
             outs=(fake,) * 5):
        return lib.gsr_keypoints(mode, B, H, W, C, r, thr, border, k, cap, logits, scores, desc, st, None, work, *outs, None)

    bad = [dict(mode=2), dict(B=0), dict(C=257), dict(r=5), dict(r=-1), dict(cap=0), dict(border=-1), dict(k=-1), dict(thr=-0.1),
           dict(thr=float("nan")), dict(thr=float("inf")), dict(H=12), dict(mode=1, W=12), dict(logits=None), dict(scores=None),
           dict(desc=None), dict(st=None), dict(work=None), dict(mode=1, C=0, H=0)]
    bad += [dict(outs=tuple(None if i == j else fake for i in range(5))) for j in range(5)]
    for kw in bad:
        assert call(**kw) == -1, kw


def test_python_checks_fire_in_order_and_refuse_cpu_tensors(monkeypatch):
    from pf3plat_amd import keypoints as kp

    def no_load():
        raise AssertionError("the library was loaded before the checks were through")

    monkeypatch.setattr(_lib, "load", no_load)
    lg, ds = torch.zeros(2, 65, 3, 4), torch.zeros(2, 8, 3, 4)
    bad = [((lg, torch.zeros(2, 257, 3, 4)), {}, "C <= 256"), ((lg, ds), {"nms_radius": 5}, "nms_radius"), ((lg, ds), {"capacity": 0}, "capacity"),
           ((lg, ds[:1]), {}, "expected descriptors"), ((lg, torch.zeros(2, 8, 4, 4)), {}, "cells"), ((lg[:, :64], ds), {}, "expected logits"),
           ((lg, ds, torch.ones(3, 2)), {}, "expected scales"), ((lg, ds), {"detection_threshold": -1.0}, "detection_threshold"),
           ((lg, ds), {"max_num_keypoints": 0}, "max_num_keypoints"), ((lg, ds), {"remove_borders": -1}, "remove_borders"),
           ((lg, ds[:, :0]), {}, "C <= 256")]
    for args, kw, word in bad:  # CPU tensors all of them: the shapes are judged first
        with pytest.raises(ValueError, match=word):
            kp.detect_keypoints(*args, **kw)
    for args, kw, word in (((torch.zeros(2, 20, 30), ds), {}, "multiples of 8"), ((torch.zeros(20, 30),), {}, "expected scores"),
                           ((torch.zeros(2, 24, 32),), {"nms_radius": 5}, "nms_radius"), ((torch.zeros(2, 24, 40), ds), {}, "cells")):
        with pytest.raises(ValueError, match=word):
            kp.keypoints_from_scores(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kp.detect_keypoints(lg, ds)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kp.keypoints_from_scores(torch.zeros(2, 20, 30))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kp.SuperPoint()({"image": torch.zeros(1, 3, 16, 24)})
    got = kp.Keypoints(torch.zeros(8, 2), torch.zeros(8, 2, dtype=torch.int32), torch.zeros(8), None, torch.tensor([3, 5], dtype=torch.int32), 4, (8, 8))
    with pytest.raises(RuntimeError, match="has 5 keypoints, capacity is 4"):
        got.lengths()
    assert got._replace(capacity=5).lengths() == (3, 5) and got._replace(capacity=5, max_num_keypoints=4).lengths() == (3, 4)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"
HOST_KEYS = ("pixels", "keypoints", "keypoint_scores", "descriptors")


def to_host(got):
    return [{k: (None if r[k] is None else r[k].cpu()) for k in HOST_KEYS} for r in got.lists()]


@functools.lru_cache(maxsize=None)
def hip_logits(name, channels_last=False):
    from pf3plat_amd import detect_keypoints

    logits, desc, scales, p = ref.logit_case(name)
    d = desc.to(DEV)
    if channels_last:
        d = d.contiguous(memory_format=torch.channels_last)
    got = detect_keypoints(logits.to(DEV), d, None if scales is None else scales.to(DEV), capacity=512, **p)
    return to_host(got), got.counts.cpu().tolist()


def same_bits(a, b):
    return all((x[k] is None and y[k] is None) or torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in HOST_KEYS) and len(a) == len(b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", tuple(ref.LOGIT_CASES))
def test_hip_matches_the_float64_restatement(name):
    got, counts = hip_logits(name)
    r64, r32 = ref.logit_reference(name)
    scales = ref.logit_case(name)[2]
    assert counts == [r["count"] for r in r64]
    for g, r in zip(got, r64):
        assert torch.equal(g["pixels"].long(), r["pixels"])  # which pixels, and in which order
    assert same_bits(got, hip_logits(name, channels_last=True)[0])  # either memory format: the same bits
    if sum(counts) == 0:
        return
    for key, floor in (("keypoint_scores", ref.FLOOR_SCORES), ("descriptors", ref.FLOOR_DESCRIPTORS)):
        err = ref.rel_l2(cat(got, key), cat(r64, key))
        bar = max(floor, 4.0 * ref.rel_l2(cat(r32, key), cat(r64, key)))
        print(f"{name}: {key} rel-L2 {err:.3e}, bar {bar:.3e}")
        assert err <= bar <= ref.CAP, (name, key)
    for b, (g, r) in enumerate(zip(got, r64)):
        s = torch.ones(2, dtype=F64) if scales is None else scales[b].double()
        bound = 2.0 ** -22 * (r["pixels"].double() + 0.5) / s
        ratio = ((g["keypoints"].double() - r["keypoints"]).abs() / bound).max() if g["keypoints"].numel() else 0.0
        print(f"{name}[{b}]: rescaled keypoints at {float(ratio):.3f} of their bound")
        assert ratio <= 1.0
        if scales is None:
            assert torch.equal(g["keypoints"], g["pixels"].float())


def hip_scores(s, **kw):
    from pf3plat_amd import keypoints_from_scores

    got = keypoints_from_scores(s.to(DEV), **kw)
    return to_host(got), got.counts.cpu().tolist()


def assert_selected(got, counts, want):
    assert counts == [n for _, _, n in want]
    for g, (pix, sc, _) in zip(got, want):
        assert torch.equal(g["pixels"].long(), pix) and torch.equal(g["keypoint_scores"], sc) and torch.equal(g["keypoints"], pix.float())


@pytest.mark.gpu
@pytest.mark.parametrize("name", tuple(ref.SCORE_CASES))
def test_hip_scores_form_is_exact(name):
    """Seeded score maps, continuous and in eighths (many ties), at sizes that are no multiples of 8 and straddle TILE: the pixels, their
    order, the counts and the scores EQUAL the restatement's, and the pixels are those of the reference's own simple_nms."""
    _, B, H, W, _, r = ref.SCORE_CASES[name]
    s = ref.score_case(name)
    record = ref.unpack_mask("nms." + name, (B, H, W))
    for border, thr in ((4, ref.THRESHOLD), (0, 0.0), (1, 0.5)):
        kw = dict(nms_radius=r, remove_borders=border, detection_threshold=thr)
        got, counts = hip_scores(s, capacity=H * W, **kw)
        assert_selected(got, counts, ref.select(s, **kw))
        for b, g in enumerate(got):
            mask = torch.zeros(H, W, dtype=torch.bool)
            mask[g["pixels"][:, 1].long(), g["pixels"][:, 0].long()] = True
            inner = torch.zeros(H, W, dtype=torch.bool)
            inner[border:H - border, border:W - border] = True
            assert torch.equal(mask, record[b] & inner & (s[b] > thr))


@pytest.mark.gpu
@pytest.mark.parametrize("direction", ("h", "v", "d"))
def test_hip_staircase_crosses_every_tile_edge_phase(direction):
    """Six descending stairs spaced 4 apart, with and without the first, from every start offset 0 ... TILE + 24: every stair meets every
    phase of a tile edge.  A pixel's result depends on scores 20 pixels away: stairs 0, 2, 4 are kept, without the first 1, 3, 5."""
    s, want = ref.staircase(direction)
    got, counts = hip_scores(s, remove_borders=0, capacity=8)
    assert counts == [3] * len(want)
    assert [[tuple(p) for p in g["pixels"].tolist()] for g in got] == [sorted(w, key=lambda p: (p[1], p[0])) for w in want]
    assert_selected(got, counts, ref.select(s, remove_borders=0))


@pytest.mark.gpu
def test_hip_top_k_cuts_in_a_fixed_order():
    """k just below, at and above the counts (36 and 35), equal scores planted inside cells: the k highest in descending order, ties to
    the lower row-major index - exactly, in the scores form on the float32 scores, and in the logits form against float64."""
    from pf3plat_amd import detect_keypoints

    logits, desc, _, p = ref.logit_case("topk")
    r64 = ref.logit_reference("topk")[0]
    n0, n1 = (r["count"] for r in r64)
    assert (n0, n1) == (36, 35)
    s32 = ref.scores_from_logits(logits, F32)
    for k in (1, 7, 34, 35, 36, 37):
        q = dict(p, max_num_keypoints=k)
        got, counts = hip_scores(s32, capacity=64, **q)
        assert_selected(got, counts, ref.select(s32, **q))
        dev = detect_keypoints(logits.to(DEV), desc.to(DEV), capacity=max(n0, n1), **q)
        want, want32 = ref.detect(logits, desc, None, q, F64), ref.detect(logits, desc, None, q, F32)
        assert dev.counts.cpu().tolist() == [n0, n1] and dev.lengths() == (min(k, n0), min(k, n1))
        for g, r, r32 in zip(to_host(dev), want, want32):
            assert torch.equal(g["pixels"].long(), r["pixels"])
            if k < r["count"]:
                assert bool((g["keypoint_scores"][1:] <= g["keypoint_scores"][:-1]).all())
            for key, floor in (("keypoint_scores", ref.FLOOR_SCORES), ("descriptors", ref.FLOOR_DESCRIPTORS)):
                bar = max(floor, 4.0 * ref.rel_l2(r32[key], r[key]))
                assert ref.rel_l2(g[key], r[key]) <= bar <= ref.CAP, (k, key)


@pytest.mark.gpu
@pytest.mark.parametrize("C", (0, 8))
def test_hip_overflow_writes_nothing_past_the_capacity(C):
    """Through ctypes, guard rows behind each buffer - with C = 8 the descriptors' too -: capacity = the larger count - 1.  The overflowing image keeps its first `capacity`
    pixels, the other image follows them, nothing is written from the total on, counts are the true counts; lengths() raises, naming the
    count; capacity = count succeeds."""
    from pf3plat_amd import _call, keypoints_from_scores

    s = ref.score_case("u37x61")[:, :32, :56].contiguous()  # (multiples of 8: the descriptors' cells)
    B, H, W = s.shape
    want = ref.select(s)
    true = [n for _, _, n in want]
    assert true == [31, 28]
    big = max(true)
    over = true.index(big)
    cap, guard = big - 1, 7
    assert min(true) < cap
    dev = s.to(DEV)
    rows = B * cap + guard
    kpts = torch.full((rows, 2), -7.0, device=DEV)
    pixels = torch.full((rows, 2), -7, dtype=torch.int32, device=DEV)
    scores = torch.full((rows,), -7.0, device=DEV)
    counts = torch.full((B + guard,), -7, dtype=torch.int32, device=DEV)
    desc = torch.randn(B, C, H // 8, W // 8, generator=ref.gen(8)) if C else None
    desc_dev = desc.to(DEV) if C else None
    out_desc = torch.full((rows, C), -7.0, device=DEV) if C else None
    strides = (ctypes.c_int64 * 4)(*desc_dev.stride()) if C else None
    work = _call.scratch(_lib.load().gsr_keypoints_scratch_bytes(B, H, W, C, cap), torch.int32, dev.device)
    _call.launch("gsr_keypoints", dev.device, 1, B, H, W, C, 4, ref.THRESHOLD, 4, 0, cap, None, dev.data_ptr(), _call.ptr(desc_dev), strides, None,
                 work.data_ptr(), kpts.data_ptr(), pixels.data_ptr(), scores.data_ptr(), _call.ptr(out_desc), counts.data_ptr())
    assert counts.cpu().tolist() == true + [-7] * guard
    stored = [min(n, cap) for n in true]
    total = sum(stored)
    assert total < B * cap
    expect = torch.cat([pix[:n] for (pix, _, _), n in zip(want, stored)])
    assert torch.equal(pixels[:total].cpu().long(), expect) and torch.equal(kpts[:total].cpu(), expect.float())
    assert torch.equal(scores[:total].cpu(), torch.cat([sc[:n] for (_, sc, _), n in zip(want, stored)]))
    assert bool((pixels[total:] == -7).all()) and bool((kpts[total:] == -7).all()) and bool((scores[total:] == -7).all())
    if C:
        assert bool((out_desc[total:] == -7).all())
        sampled = lambda dtype: torch.cat([ref.sample(pix[:n], desc[b], dtype) for b, ((pix, _, _), n) in enumerate(zip(want, stored))])
        err = ref.rel_l2(out_desc[:total].cpu(), sampled(F64))
        bar = max(ref.FLOOR_DESCRIPTORS, 4.0 * ref.rel_l2(sampled(F32), sampled(F64)))
        print(f"overflow, C = {C}: descriptors rel-L2 {err:.3e}, bar {bar:.3e}")
        assert err <= bar <= ref.CAP
    with pytest.raises(RuntimeError, match=f"image {over} has {big} keypoints, capacity is {cap}"):
        keypoints_from_scores(dev, capacity=cap).lengths()
    ok = keypoints_from_scores(dev, capacity=big)
    assert ok.lengths() == tuple(true)
    assert_selected(to_host(ok), ok.counts.cpu().tolist(), want)


@pytest.mark.gpu
def test_hip_repeats_bit_for_bit_and_images_do_not_touch_one_another():
    from pf3plat_amd import detect_keypoints

    logits, desc, scales, p = ref.logit_case("batch")
    run = lambda sel: to_host(detect_keypoints(logits[sel].to(DEV), desc[sel].to(DEV), scales[sel].to(DEV), capacity=512, **p))
    whole = run(slice(None))
    assert same_bits(whole, run(slice(None))) and same_bits(whole, hip_logits("batch")[0])
    for b in range(logits.shape[0]):
        assert same_bits(whole[b:b + 1], run(slice(b, b + 1))), b


@pytest.mark.gpu
@pytest.mark.parametrize("name", tuple(ref.SCAN_CASES))
def test_hip_scan_carries_its_count_past_2048_words(name):
    """One image of 2048, 2049 and 2080 mask words, in eighths: pixels, order, count and scores equal the restatement's."""
    s, kw, want = ref.scan_case(name)
    got, counts = hip_scores(s, capacity=s.shape[1] * s.shape[2], **kw)
    print(f"scan {name}: {counts[0]} keypoints")
    assert_selected(got, counts, want)


BATCH_ROWS = 16  # the capacity of the 260-image calls: rows an image may fill


@functools.lru_cache(maxsize=None)
def hip_batch(form):
    s, desc, kw = ref.batch_case()
    k, C = ref.BATCH_CASE[7:]
    kw = dict(kw, max_num_keypoints=k) if form == "cut" else kw
    got, counts = hip_scores(s, **({"descriptors": desc.to(DEV)} if form == "descriptors" else {}), capacity=BATCH_ROWS, **kw)
    return got, counts, ref.select(s, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("plain", "cut", "descriptors"))
def test_hip_batch_of_260_images_sums_the_rows_before_an_image_past_256(form):
    """260 images of 8 x 8, some empty: as they are found (the write pass forms the first row of the images from 257 on), cut to the
    2 highest (those images are staged: the top-k pass forms it), with descriptors (the descriptor pass does; one cell an image, so a
    keypoint's descriptor is its image's normalised cell and names the image the row was taken for)."""
    got, counts, want = hip_batch(form)
    assert max(counts) <= BATCH_ROWS  # (no image overflows the capacity)
    assert_selected(got, counts, want)
    if form == "descriptors":
        desc = ref.batch_case()[1]
        sampled = lambda dtype: torch.cat([ref.sample(pix, desc[b], dtype) for b, (pix, _, _) in enumerate(want)])
        err = ref.rel_l2(cat(got, "descriptors"), sampled(F64))
        bar = max(ref.FLOOR_DESCRIPTORS, 4.0 * ref.rel_l2(sampled(F32), sampled(F64)))
        last = ref.rel_l2(torch.cat([g["descriptors"] for g in got[ref.BASE_STEP + 1:]]),
                          torch.cat([ref.sample(pix, desc[b], F64) for b, (pix, _, _) in enumerate(want) if b > ref.BASE_STEP]))
        print(f"batch of {len(got)}: descriptors rel-L2 {err:.3e}, of the images past {ref.BASE_STEP} {last:.3e}, bar {bar:.3e}")
        assert err <= bar <= ref.CAP and last <= bar
    else:
        assert all(g["descriptors"] is None for g in got)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("plain", "cut", "descriptors"))
def test_hip_image_258_alone_has_the_rows_it_has_in_the_batch(form):
    s, desc, kw = ref.batch_case()
    k, C = ref.BATCH_CASE[7:]
    kw = dict(kw, max_num_keypoints=k) if form == "cut" else kw
    b = ref.BASE_STEP + 2
    alone, counts = hip_scores(s[b:b + 1], **({"descriptors": desc[b:b + 1].to(DEV)} if form == "descriptors" else {}), capacity=BATCH_ROWS, **kw)
    assert counts == hip_batch(form)[1][b:b + 1] and counts[0] > k and same_bits(alone, hip_batch(form)[0][b:b + 1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", tuple(ref.TOPK_CASES))
def test_hip_top_k_ranks_past_a_chunk_of_8192(name):
    """8192, 8193 and 17394 keypoints found of eight distinct scores, the cut between half of them and all: the kept ones, in
    descending order with ties to the lower row-major index, equal the restatement's stable sort."""
    s, kw, want, _ = ref.topk_case(name)
    got, counts = hip_scores(s, capacity=s.shape[1] * s.shape[2], **kw)
    print(f"top-k {name}: {counts[0]} found, {len(got[0]['pixels'])} kept")
    assert len(got[0]["pixels"]) == kw["max_num_keypoints"] < counts[0]
    assert_selected(got, counts, want)


@pytest.mark.gpu
def test_hip_packed_keypoints_feed_the_match_assignment():
    """`packed()` goes straight into the ragged match assignment: ids_i is y * width + x of the detected pixels."""
    from pf3plat_amd import detect_keypoints, match_assignment

    logits, desc, _, p = ref.logit_case("batch")
    got = detect_keypoints(logits.to(DEV), desc.to(DEV), capacity=512, **p)
    packed = got.packed()
    assert packed.lengths == (346, 0, 337) and packed.keypoints.shape[0] == sum(packed.lengths)
    g = torch.Generator().manual_seed(3)
    mdesc = packed.descriptors + 0.05 * torch.randn(packed.descriptors.shape, generator=g).to(DEV)
    z = torch.full((sum(packed.lengths),), 4.0, device=DEV)
    width = got.size[1]
    m = match_assignment(3.0 * packed.descriptors, 3.0 * mdesc, z, z, packed.lengths, packed.lengths, threshold=0.1, scale=1.0,
                         kpts0=packed.keypoints, kpts1=packed.keypoints, width=width)
    counts = m.counts.cpu().tolist()
    assert counts[1] == 0 and counts[0] > 300 and counts[2] > 300
    pix = packed.pixels.long()
    for l, c in enumerate(counts):
        o = m.offsets0[l]
        rows = m.idx0[o:o + c].long() + o
        assert torch.equal(m.ids_i[o:o + c], pix[rows, 1] * width + pix[rows, 0])
        assert torch.equal(m.idx0[o:o + c], m.idx1[o:o + c])  # a noisy copy of itself matches itself


@pytest.mark.gpu
def test_hip_superpoint_module_runs_its_head_on_the_device():
    from pf3plat_amd import SuperPoint, detect_keypoints

    module = SuperPoint(capacity=256)
    module.load_state_dict(reference_state())
    module = module.to(DEV).eval()
    image = torch.rand(2, 3, 48, 64, generator=ref.gen(6)).to(DEV)
    scales = torch.tensor([[1.0, 1.0], [0.5, 0.8]], device=DEV)
    seen, heads = [], module.heads
    module.heads = lambda x: seen.append(heads(x)) or seen[-1]  # the module's own convolutions' outputs, as its forward saw them
    got = module({"image": image, "scales": scales})
    (logits, desc), = seen
    assert tuple(logits.shape) == (2, 65, 6, 8) and tuple(desc.shape) == (2, 256, 6, 8)
    grey = (image * torch.tensor([0.299, 0.587, 0.114], device=DEV).view(1, 3, 1, 1)).sum(1, keepdim=True)
    assert torch.allclose(heads(grey)[0], logits, atol=1e-3) and torch.allclose(heads(grey)[1], desc, atol=1e-3)  # RGB to grey, by those weights
    want = detect_keypoints(logits, desc, scales, capacity=256)
    assert sum(got.lengths()) > 0 and got.lengths() == want.lengths() and same_bits(to_host(got), to_host(want))
