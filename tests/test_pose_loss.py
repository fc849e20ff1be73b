"""The pose loss on the device (gsr_pose_loss / gsr_pose_loss_backward; pf3plat_amd.losses.pose_loss, Losspose) against its torch
restatement tests/pose_loss_ref.py.  CPU: the float64 restatement against numbers recorded from the reference's own Losspose
(tests/golden/pose_loss_fixtures.npz), the host side of the three C entry points, the Python argument checks, and the conditions the
GPU cases rely on (both sides of the Huber threshold populated; every bar under the project's 1e-4).  GPU: value and the three
gradients of every case against the float64 restatement, the bar tied to what the SAME restatement loses in float32; the rows of
`lists` and the two logged means of the larger cases against float64, list by list, through the C entry point.

The first eight cases end every reduction loop of the four kernels in one trip.  The others are there for the further trips:
  l16      16 lists: k_pose_loss_finish's loop over blocks of 16 lists runs once, full to its last wave;
  l17      17 lists: a second block that holds one list, which finds its rows behind `first += total` of block 0; list 15, the last
           wave of block 0, is empty;
  train42  42 lists of about 1000 matches (the training batch's count, 14 scenes x 3 pairs): three blocks, `first` carried twice,
           `before` inside a block over lists of 3 to 6 units, lengths 0 / 1024 / 1023 / 1025 on the two block edges;
  b7v5     70 lists, five views: the final sum over lists (l = lane, lane + 64) takes a second trip for lists 64 .. 69, as does
           k_pose_loss_pose_reduce's count of the units in front of list l for l >= 65; pose_pair_of for ten pairs, i up to 3;
  long     lists of 16 641 and 16 384 matches: 66 units (lane k of the finish adds rows k and k + 64) beside exactly 64 (one trip);
  signed   scores of both signs: the L1 norm is of |score|;
  wide     200 x 328 pixels: ids above 2^16, the first and the last pixel, / and % by a width that is no power of two."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import pose_loss_ref as ref

H, W = 12, 20  # unequal, so that % and // by the wrong extent show
WEIGHT_2D, WEIGHT_3D = 0.3, 1.7
K_OWN = 4.0  # tests/test_losses.py: another order of the same float32 operations has the same order of rounding, other bits
# What the float32 restatement loses against the float64 one, worst case over CASES (measured on the CPU, docs/PARITY.md):
# value 2.20e-6 (one_pixel), dL/dxyz 3.89e-6 (v4), dL/ddepth 2.49e-6 (fixture), dL/dposes 2.03e-5 (v2: on the quadratic side of the
# Huber term the gradient is a difference of two coordinates near 0.5 that agree to 1e-3).  A single case can land closer than
# that by chance, and its bar should not follow it down: the floor is that worst case, rounded up in its second digit.  (The
# figures move in their second digit with the host's BLAS; the floor is a constant, a case's own 4 x term is computed where it runs.)
FLOOR = {"value": 2.3e-6, "xyz": 3.9e-6, "depth": 2.5e-6, "poses": 2.1e-5}
CAP = 1e-4  # the project's bar: no case's may be wider - an input that needs more is badly chosen
EDGE_LENGTHS = (0, 1, 7, 63, 64, 65, 255, 256, 257, 700, 130, 0)  # wave and unit edges, several units in a list
MIXED = ("random", "random", "near")  # kinds by scene, s % 3
# name -> build_scene arguments (seed, b, v, lengths, kinds, ...; h, w where they are not H, W)
CASES = {
    # scene 1 "random": poses[1, 0] is a general matrix, which the i == 0 shortcut must not read
    "b2v3": dict(seed=1, b=2, v=3, lengths=(65, 0, 256, 7, 130, 63), kinds=("near", "random")),
    "v2": dict(seed=2, b=3, v=2, lengths=(257, 1, 64), kinds=("near", "random", "near")),
    "v4": dict(seed=3, b=2, v=4, lengths=EDGE_LENGTHS, kinds=("random", "near")),  # six pairs, a view in three of them
    "empty": dict(seed=4, b=2, v=3, lengths=(0,) * 6, kinds=("near", "random")),
    "zero_weights": dict(seed=5, b=1, v=3, lengths=(70, 40, 9), kinds=("random",), zero_weight_lists=(0,)),
    "one_pixel": dict(seed=6, b=1, v=3, lengths=(300, 5, 70), kinds=("random",), repeat_lists=(0, 2)),
    "zero_residual": dict(seed=7, b=1, v=2, lengths=(100,), kinds=("random",), exact=True),  # 3D residuals exactly 0
    "fixture": dict(seed=77, b=2, v=3, lengths=(0, 1, 7, 64, 65, 130), kinds=("near", "random")),  # make_pose_loss_fixtures.py's
    # the loops past their first trip (the header says which).  Seeds: among ~20 000 unrelated id pairs a few reproject within 0.01 of
    # their partner by chance; each seed is the first from the case's own number (16, 17, 42, 75, 8, 9, 10) that leaves every match at
    # least 1e-4 on its scene's side of the Huber threshold in float64.  l16, l17: 15 and 16 units
    "l16": dict(seed=17, b=16, v=2, lengths=(0, 1, 255, 256, 257, 65, 0, 1, 255, 256, 257, 65, 0, 1, 255, 256), kinds=(MIXED * 6)[:16]),
    "l17": dict(seed=18, b=17, v=2, lengths=(0, 1, 255, 256, 257, 65, 0, 1, 255, 256, 257, 65, 0, 1, 255, 0, 300), kinds=(MIXED * 6)[:17]),
    # 184 units; lists 15 | 16 and 31 | 32 lie on the block edges
    "train42": dict(seed=65, b=14, v=3, h=32, w=48, kinds=("random", "near") * 7,
                    lengths=(1056, 1199, 940, 1036, 870, 827, 1210, 1010, 1378, 755, 1135, 748, 1166, 1059, 789, 0,
                             1024, 1243, 1278, 838, 775, 797, 610, 749, 1337, 1288, 1178, 1194, 1141, 1375, 756, 1023,
                             1025, 841, 986, 1075, 647, 1316, 1060, 765, 827, 1300)),
    # 74 units; the cycle 0, 1, 7, 63, 64, 65, 255, 256, 257 up to list 63, then lists 64 .. 69 of 2, 1, 3, 1, 3 and 1 units
    "b7v5": dict(seed=75, b=7, v=5, kinds=("random", "random", "near", "random", "random", "near", "random"),
                 lengths=(0, 1, 7, 63, 64, 65, 255, 256, 257) * 7 + (0, 257, 65, 700, 7, 513, 256)),
    "long": dict(seed=16, b=2, v=2, h=96, w=176, lengths=(16641, 16384), kinds=("random", "near")),  # 66 and 64 units
    "signed": dict(seed=10, b=1, v=3, lengths=(70, 257, 9), kinds=("random",), signed_lists=(0, 1, 2)),
    "wide": dict(seed=10, b=1, v=2, h=200, w=328, lengths=(600,), kinds=("random",), corner_lists=(0,)),
}
LIST_CASES = ("l17", "train42", "b7v5", "long")  # the cases whose rows of `lists` are compared one by one
QUANTITIES = ("value", "xyz", "depth", "poses")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_loss_fixtures.npz")


@functools.lru_cache(maxsize=None)
def scene(name):
    return ref.build_scene(**{"h": H, "w": W, **CASES[name]})


@functools.lru_cache(maxsize=None)
def restated(name, dtype):
    """-> {"value", "xyz", "depth", "poses"}: the restatement's loss and gradients as float64 numpy; computed once and shared."""
    sc = scene(name)
    xyz, depth, poses = (t.clone().requires_grad_(True) for t in (sc.xyz, sc.depth, sc.poses))
    loss, _, _ = ref.pose_loss(xyz, depth, poses, sc.intrinsics, sc.corr, sc.conf, WEIGHT_2D, WEIGHT_3D, dtype)
    assert loss.dtype == dtype
    loss.backward()
    return {"value": loss.detach().double().numpy(), "xyz": xyz.grad.double().numpy(), "depth": depth.grad.double().numpy(),
            "poses": poses.grad.double().numpy()}


def distance(got, want):
    """|got - want| / |want| (rel-L2 for arrays); a reference that is exactly zero asks for exact zeros."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    norm = np.linalg.norm(want)
    return float(np.linalg.norm(got - want) / norm) if norm > 0 else (0.0 if not np.any(got) else np.inf)


def own_error(name):
    r64, r32 = restated(name, torch.float64), restated(name, torch.float32)
    return {q: distance(r32[q], r64[q]) for q in QUANTITIES}


def bars(name):
    return {q: max(FLOOR[q], K_OWN * e) for q, e in own_error(name).items()}


@functools.lru_cache(maxsize=None)
def restated_lists(name, dtype):
    """-> (rows, m3, m2): the rows of `lists` as include/gsr.h defines them - (conf x L3 term, L2 term, w3d x conf / (max(sum |w|,
    1e-12) x L), sum |w|), list order pair-major then scene - from the restatement's per-list terms and the inputs, and the two
    logged means; everything computed in `dtype`, returned as float64 numpy."""
    sc = scene(name)
    with torch.no_grad():
        _, m3, m2, (l3, l2, sw) = ref.pose_loss(sc.xyz, sc.depth, sc.poses, sc.intrinsics, sc.corr, sc.conf, WEIGHT_2D, WEIGHT_3D, dtype, per_list=True)
    b, v = sc.xyz.shape[:2]
    cf = torch.stack([sc.conf[p][s] for p in ref.pairs_of(v) for s in range(b)]).to(dtype)
    factor = torch.tensor(WEIGHT_3D, dtype=dtype) * cf / (sw.clamp_min(1e-12) * len(cf))
    rows = torch.stack([l3, l2, factor, sw], -1)
    assert rows.dtype == dtype and rows.shape == (len(CASES[name]["lengths"]), 4)
    return rows.double().numpy(), float(m3), float(m2)


def per_entry(got, want):
    """|got - want| / |want| entry by entry; where the reference is exactly zero: 0 for an exact zero, inf for anything else."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got == 0, 0.0, np.inf))


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_float64_restatement_against_the_recorded_reference_numbers():
    """The reference's own Losspose ran in float32 (tests/golden/make_pose_loss_fixtures.py); the issue's probe put float32 against
    float64 of the reference itself at 4e-7 (value) and up to 4e-6 (gradients), so the restatement has to be within 2e-5 of the
    record - several times that and far below any misreading of the definition - and the fixture's inputs are the scene builder's."""
    f = np.load(FIXTURE)
    sc = scene("fixture")
    for key, t in (("xyz", sc.xyz), ("depth", sc.depth), ("poses", sc.poses), ("intrinsics", sc.intrinsics)):
        assert np.array_equal(f[key], t.numpy()), key
    assert tuple(f["weights"]) == (np.float32(WEIGHT_2D), np.float32(WEIGHT_3D))
    r64 = restated("fixture", torch.float64)
    figures = {"value": distance(r64["value"], f["value"]), "xyz": distance(r64["xyz"], f["grad_xyz"]),
               "depth": distance(r64["depth"], f["grad_depth"]), "poses": distance(r64["poses"][:, :, :3], f["grad_poses_top"])}
    print("[pose] float64 restatement vs the reference's record:", {k: f"{v:.1e}" for k, v in figures.items()})
    assert all(v <= 2e-5 for v in figures.values()), figures
    assert not np.any(r64["poses"][:, :, 3])  # the bottom row is a constant
    # the loop form (what tools/pose_loss_prof.py times) is the same loss; it normalises the float32 scores where they lie, as the
    # reference does, hence a few float32 roundings (6e-8 each) averaged over the matches and not 1e-16
    loop = ref.pose_loss_loop(sc.xyz.double(), sc.depth.double(), sc.poses.double(), sc.intrinsics.double(), sc.corr, sc.conf, WEIGHT_2D, WEIGHT_3D)
    assert abs(float(loop[0]) - float(r64["value"])) <= 1e-7 * float(r64["value"])


def test_cases_populate_both_sides_of_the_huber_threshold_and_bars_stay_under_the_cap():
    """In float64: the near-identity scenes put every reprojection residual on the quadratic side of delta = 0.01, the random-id
    scenes on the linear side, both sides hold matches in each mixed case; the exact case has 3D residuals that are exactly 0.  And no
    bar of any case is wider than 1e-4."""
    for name, args in CASES.items():
        sc = scene(name)
        r3, r2, lid = ref.residuals((sc.xyz, sc.depth, sc.poses, sc.intrinsics, sc.corr))
        near = torch.tensor([args["kinds"][int(l) % args["b"]] == "near" for l in lid], dtype=torch.bool)
        assert bool((r2[near] <= ref.DELTA).all()) and bool((r2[~near] > ref.DELTA).all()), name
        if len(set(args["kinds"])) == 2 and len(r2):
            assert int(near.sum()) > 0 and int((~near).sum()) > 0, name
        if args.get("exact"):
            assert len(r3) == 100 and not bool(r3.any())
        own, bar = own_error(name), bars(name)
        print(f"[pose] {name:13s} quadratic {int((r2 <= ref.DELTA).sum()):4d} linear {int((r2 > ref.DELTA).sum()):4d}   float32 vs float64: "
              + "  ".join(f"{q} {own[q]:.1e}" for q in QUANTITIES))
        assert all(b <= CAP for b in bar.values()), (name, bar)
    assert sorted(set(CASES["v4"]["lengths"])) == [0, 1, 7, 63, 64, 65, 130, 255, 256, 257, 700]
    sc = scene("signed")  # both signs in every list, and an L1 norm that is nowhere near the clamp at 1e-12
    for p in ref.pairs_of(3):
        score = sc.corr[p][0][2]
        assert bool((score < 0).any()) and bool((score > 0).any()) and float(score.abs().min()) >= 0.05 and float(score.abs().sum()) > 1, p
        assert abs(float(score.sum())) < 0.75 * float(score.abs().sum()), p  # a sum without the absolute value is another number
    sc = scene("wide")
    a, c, _ = sc.corr[(0, 1)][0]
    assert (sc.xyz.shape[-2:], a[:2].tolist(), c[:2].tolist()) == ((200, 328), [0, 200 * 328 - 1], [200 * 328 - 1, 0]) and 200 * 328 > 1 << 16


def test_pose_loss_symbols_unit_count_and_argument_errors():
    """The three entry points are declared in include/gsr.h and exported (ABI 5 as before); gsr_pose_loss_units is host arithmetic;
    every argument error returns GSR_ERR_INVALID_ARGUMENT before anything is launched (there is no device here: a call that got past
    its checks would return the launch error instead)."""
    from pf3plat_amd import _lib

    lib = _lib.load()
    assert lib.gsr_abi_version() == 5 == _lib.GSR_ABI_VERSION
    exported = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    for name in ("gsr_pose_loss", "gsr_pose_loss_backward", "gsr_pose_loss_units"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(exported, name) and f"{name}(" in header, name
    arr = lambda *v: (ctypes.c_int32 * len(v))(*v)
    units = lambda *v: lib.gsr_pose_loss_units(len(v) - 1, arr(*v))
    assert units(0) == 0 and units(0, 0, 0) == 0 and units(0, 1) == 1 and units(0, 256) == 1 and units(0, 257) == 2
    assert units(*np.cumsum((0,) + EDGE_LENGTHS).tolist()) == 0 + 1 + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 3 + 1 + 0 == 13
    assert units(5, 5, 261, 1000) == 0 + 1 + 3  # a start other than 0 is allowed
    of_case = lambda name: units(*np.cumsum((0,) + CASES[name]["lengths"]).tolist())
    assert (of_case("l16"), of_case("l17"), of_case("train42"), of_case("b7v5"), of_case("long")) == (15, 16, 184, 74, 66 + 64)
    assert [len(CASES[n]["lengths"]) for n in ("l16", "l17", "train42", "b7v5", "long")] == [16, 17, 42, 70, 2]
    assert units(0, *np.cumsum(CASES["b7v5"]["lengths"][:64]).tolist()) == 63 and units(0, *np.cumsum(CASES["b7v5"]["lengths"][64:]).tolist()) == 11
    assert CASES["l17"]["lengths"][15:] == (0, 300) and all(n > 0 for n in CASES["b7v5"]["lengths"][64:])
    t42 = CASES["train42"]["lengths"]
    assert (t42[15], t42[16], t42[31], t42[32]) == (0, 1024, 1023, 1025) and t42[41] > 4 * 256 and 950 < sum(t42) / 42 < 1050
    assert units(0, 3, 2) == -1 and units(-1, 3) == -1 and lib.gsr_pose_loss_units(1, None) == -1 and lib.gsr_pose_loss_units(-1, arr(0)) == -1
    invalid = -1  # GSR_ERR_INVALID_ARGUMENT of include/gsr.h
    p = ctypes.c_void_p(4096)  # a non-null address that is never read: every call below returns before its launch
    good = dict(b=2, v=3, h=H, w=W, pairs=3, xyz=p, depth=p, poses=p, intr=p, ids_i=p, ids_j=p, wgt=p, conf=p, offs=arr(0, 1, 2, 3, 4, 5, 300),
                offs_dev=p, partials=p, lists=p, out=p, up=p, d_xyz=p, d_depth=p, d_poses=p)

    def forward(**change):
        a = {**good, **change}
        return lib.gsr_pose_loss(a["b"], a["v"], a["h"], a["w"], a["pairs"], a["xyz"], a["depth"], a["poses"], a["intr"], a["ids_i"], a["ids_j"],
                                 a["wgt"], a["conf"], a["offs"], a["offs_dev"], 1.0, 1.0, a["partials"], a["lists"], a["out"], None)

    def backward(**change):
        a = {**good, **change}
        return lib.gsr_pose_loss_backward(a["b"], a["v"], a["h"], a["w"], a["pairs"], a["xyz"], a["depth"], a["poses"], a["intr"], a["ids_i"],
                                          a["ids_j"], a["wgt"], a["conf"], a["offs"], a["offs_dev"], 1.0, 1.0, a["lists"], a["up"], a["d_xyz"],
                                          a["d_depth"], a["d_poses"], a["partials"], None)

    shared = ("xyz", "depth", "poses", "intr", "ids_i", "ids_j", "wgt", "conf", "offs", "offs_dev", "partials", "lists")
    for call, own in ((forward, ("out",)), (backward, ("up", "d_xyz", "d_depth", "d_poses"))):
        for name in shared + own:
            assert call(**{name: None}) == invalid, (call.__name__, name)
        assert call(offs=arr(0, 1, 2, 3, 2, 5, 300)) == invalid  # not monotone
        assert call(offs=arr(-1, 1, 2, 3, 4, 5, 300)) == invalid  # negative
        assert call(v=1, pairs=0) == invalid and call(v=0, pairs=0) == invalid
        assert call(pairs=2) == invalid and call(v=4) == invalid and call(v=4, pairs=5) == invalid
        assert call(b=-1) == invalid and call(h=0) == invalid and call(w=-3) == invalid and call(h=1 << 16, w=1 << 16) == invalid
    assert backward(b=0, offs=arr(0)) == 0  # no scene: nothing to write, nothing launched


def test_python_argument_checks_come_before_the_device_and_cpu_tensors_are_refused(monkeypatch):
    """ValueError from the shapes alone - before the device is looked at and before the library is loaded; RuntimeError for CPU
    tensors of legal shapes; packing works anywhere (it is a few torch.cat) and takes its offsets from the shapes."""
    from pf3plat_amd import _lib, losses

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    sc = scene("b2v3")
    packed = losses.pack_correspondences(sc.corr, sc.conf)
    assert packed.offsets == tuple(np.cumsum((0,) + CASES["b2v3"]["lengths"]).tolist()) and (packed.num_scenes, packed.num_pairs) == (2, 3)
    assert packed.ids_i.dtype == packed.ids_j.dtype == torch.int64 and packed.weights.dtype == packed.conf.dtype == torch.float32
    assert packed.offsets_device.dtype == torch.int32 and packed.offsets_device.tolist() == list(packed.offsets)
    order = [(p, s) for p in ref.pairs_of(3) for s in range(2)]  # pair-major, then scene
    assert torch.equal(packed.ids_j, torch.cat([sc.corr[p][s][1] for p, s in order]))
    assert torch.equal(packed.conf, torch.stack([sc.conf[p][s] for p, s in order]))
    as_lists = losses.pack_correspondences(sc.corr, {p: [float(c) for c in sc.conf[p]] for p in sc.conf})  # confidences as Python lists
    assert torch.equal(as_lists.conf, packed.conf)
    good = (sc.xyz, sc.depth, sc.poses, sc.intrinsics)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.pose_loss(*good, packed, WEIGHT_2D, WEIGHT_3D)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.pose_loss(sc.xyz, sc.depth.reshape(2, 3, H, W), sc.poses, sc.intrinsics, packed, WEIGHT_2D, WEIGHT_3D)
    bad = [(0, sc.xyz[:, :, :2], "xyz"), (0, sc.xyz[0], "xyz"), (0, sc.xyz[:, :1], "two views"), (1, sc.depth[:5], "depth"),
           (1, sc.depth.reshape(6, H, W), "depth"), (1, sc.depth.reshape(2, 3, W, H), "depth"), (2, sc.poses[:, :, :3], "poses"),
           (2, sc.poses[:1], "poses"), (3, sc.intrinsics[:, :2], "intrinsics"), (3, sc.poses, "intrinsics")]
    for at, tensor, word in bad:
        args = list(good)
        args[at] = tensor
        with pytest.raises(ValueError, match=word):
            losses.pose_loss(*args, packed, WEIGHT_2D, WEIGHT_3D)
    other = scene("v2")
    with pytest.raises(ValueError, match="packed for 3 scenes and 1 pairs"):
        losses.pose_loss(*good, losses.pack_correspondences(other.corr, other.conf), WEIGHT_2D, WEIGHT_3D)
    with pytest.raises(ValueError, match="every pair"):
        losses.pack_correspondences({(0, 1): sc.corr[(0, 1)], (1, 2): sc.corr[(1, 2)]}, sc.conf)
    with pytest.raises(ValueError, match="one list and one confidence per scene"):
        losses.pack_correspondences({**sc.corr, (1, 2): sc.corr[(1, 2)][:1]}, sc.conf)
    with pytest.raises(ValueError, match="three equal 1-D tensors"):
        losses.pack_correspondences({**sc.corr, (0, 1): [(torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(3))] * 2}, sc.conf)
    module = losses.Losspose(losses.LossposeCfg(WEIGHT_2D, WEIGHT_3D))
    batch = {"target": {"intrinsics": sc.intrinsics}}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        module(None, batch, None, 0, (None, sc.poses), (sc.depth,), (sc.corr, None, sc.conf), sc.xyz)


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


def run_hip(name, scale=1.0, transform=None):
    """-> (the three outputs, {"value", "xyz", "depth", "poses"} as torch tensors on the device) of pose_loss on a case's inputs."""
    from pf3plat_amd import losses

    sc = scene(name)
    xyz, depth, poses, intr = (t.to(DEV) for t in (sc.xyz, sc.depth, sc.poses, sc.intrinsics))
    if transform is not None:
        xyz, depth, poses, intr = transform(xyz, depth, poses, intr)
    xyz, depth, poses = (t.requires_grad_(True) for t in (xyz, depth, poses))
    corr = {p: [tuple(t.to(DEV) for t in entry) for entry in lists] for p, lists in sc.corr.items()}
    conf = {p: c.to(DEV) for p, c in sc.conf.items()}
    out = losses.pose_loss(xyz, depth, poses, intr, losses.pack_correspondences(corr, conf), WEIGHT_2D, WEIGHT_3D)
    assert all(o.dtype == torch.float32 and o.shape == () and o.device == torch.device(DEV) for o in out)
    assert out[0].requires_grad and not out[1].requires_grad and not out[2].requires_grad
    (scale * out[0]).backward()
    return out, {"value": out[0].detach(), "xyz": xyz.grad, "depth": depth.grad, "poses": poses.grad}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_pose_loss_against_float64_restatement(name):
    """Value and dL/dxyz, dL/ddepth, dL/dposes of every case: distance to the float64 restatement <= max(FLOOR, 4 x the float32
    restatement's own distance), no bar above 1e-4; the two logged means recombine to the loss; all finite (the exact case: a norm's
    gradient at 0 is 0); an all-empty call gives exact zeros."""
    out, got = run_hip(name)
    r64, own, bar = restated(name, torch.float64), own_error(name), bars(name)
    assert abs(float(out[0].detach()) - (WEIGHT_3D * float(out[1]) + WEIGHT_2D * float(out[2]))) <= 1e-6 * abs(float(out[0].detach()))
    failed = []
    for q in QUANTITIES:
        g = got[q].double().cpu().numpy().reshape(r64[q].shape)
        err = distance(g, r64[q])
        print(f"[pose] {name:13s} {q:6s} hip vs float64: {err:.3e}   float32 restatement vs float64: {own[q]:.3e}   bar: {bar[q]:.3e}")
        assert bar[q] <= CAP, (name, q, bar[q])
        if not err <= bar[q]:
            failed.append((q, err, bar[q]))
    assert not failed, (name, failed)
    assert not bool(got["poses"][:, :, 3].any())
    if name == "empty":
        assert all(not bool(got[q].any()) for q in QUANTITIES)


def run_c_forward(name):
    """gsr_pose_loss itself on a case's inputs (ctypes, as tools/pose_loss_prof.py calls it: `lists` is no output of the torch
    function) -> (lists (L, 4), out (4,)) as float64 numpy.  All three outputs start as NaN: what the kernels leave out shows."""
    from pf3plat_amd import _lib, losses
    from pf3plat_amd.rasterizer import _stream_ptr

    lib, dev = _lib.load(), torch.device(DEV)
    sc = scene(name)
    b, v, _, h, w = sc.xyz.shape
    xyz, depth, poses, intr = (t.to(dev).contiguous() for t in (sc.xyz, sc.depth, sc.poses, sc.intrinsics))
    corr = {p: [tuple(t.to(dev) for t in entry) for entry in lists] for p, lists in sc.corr.items()}
    packed = losses.pack_correspondences(corr, {p: c.to(dev) for p, c in sc.conf.items()})
    num_lists = len(packed.offsets) - 1
    host = (ctypes.c_int32 * len(packed.offsets))(*packed.offsets)
    units = int(lib.gsr_pose_loss_units(num_lists, host))
    assert num_lists == len(CASES[name]["lengths"]) and units >= 0 and packed.offsets[-1] == sum(CASES[name]["lengths"])
    nan = dict(dtype=torch.float32, device=dev)
    partials, lists, out = torch.full((max(units, 1), 4), float("nan"), **nan), torch.full((num_lists, 4), float("nan"), **nan), torch.full((4,), float("nan"), **nan)
    status = lib.gsr_pose_loss(b, v, h, w, v * (v - 1) // 2, xyz.data_ptr(), depth.data_ptr(), poses.data_ptr(), intr.data_ptr(), packed.ids_i.data_ptr(),
                               packed.ids_j.data_ptr(), packed.weights.data_ptr(), packed.conf.data_ptr(), host, packed.offsets_device.data_ptr(),
                               WEIGHT_2D, WEIGHT_3D, partials.data_ptr(), lists.data_ptr(), out.data_ptr(), _stream_ptr(dev))
    assert status == 0
    return lists.double().cpu().numpy(), out.double().cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", LIST_CASES)
def test_hip_pose_loss_rows_of_lists_and_the_two_means_against_float64(name):
    """Every row of `lists` - (conf x L3 term, L2 term, w3d x conf / (max(sum |w|, 1e-12) x L), sum |w|) - against the float64
    restatement's per-list terms and the inputs, entry by entry and relative; an entry that is exactly 0 in float64 (an empty list's
    sums) has to be exactly 0.  A list's bar is the value rule applied to that list: max(FLOOR["value"], 4 x the largest relative
    distance of the float32 restatement's row of the same list), never above 1e-4.  The value alone cannot see a unit that went to
    the wrong list - the total of the 2D term does not change - and sees a wrong 3D row only through that list's normalisation.
    out[1] and out[2] against the float64 means at the case's value bar.
    The 2D entry is what this test changed in the kernels.  In a "near" scene every 2D residual is the difference of two
    coordinates near 0.5 that agree to 1e-3; with the reprojection in float32 the kernel kept four digits of it, as the float32
    restatement does (its rows are up to 4.0e-5 from float64 in this entry), and three rows - train42 lists 33 and 37, b7v5 list 37,
    all of pairs with i > 0 - lay 4.3e-5, 2.3e-5 and 4.5e-5 from float64 against bars of 1.4e-5, 4.3e-6 and 2.1e-5: one list's own
    float32 distance is one draw from a range, the kernel's another.  pose_match now carries the reprojection from the pixel centre
    to the residual in fp64 (Rt and K_i^-1 unrounded), and the worst row of the four cases is 7.4e-6 from float64 (docs/PARITY.md 13.1)."""
    got, out = run_c_forward(name)
    (want, m3, m2), (own_rows, _, _) = restated_lists(name, torch.float64), restated_lists(name, torch.float32)
    lengths = CASES[name]["lengths"]
    units = [(n + 255) // 256 for n in lengths]
    assert got.shape == want.shape == (len(lengths), 4)
    each = per_entry(got, want)
    err, own = each.max(axis=1), per_entry(own_rows, want).max(axis=1)
    assert np.all(np.isfinite(own)), name
    bar = np.minimum(np.maximum(FLOOR["value"], K_OWN * own), CAP)
    worst = int(np.argmax(err / bar))
    entry = ("conf x L3", "L2", "3D factor", "sum |w|")[int(np.argmax(each[worst]))]
    where = f"list {worst} (block {worst // 16}, {lengths[worst]} matches in {units[worst]} units, {sum(units[:worst])} units in front of it), entry {entry}"
    print(f"[pose] {name:13s} lists   hip vs float64, worst in bars: {err[worst]:.3e} of {bar[worst]:.3e} at {where}; largest distance {err.max():.3e} "
          f"(list {int(np.argmax(err))}); float32 restatement vs float64, largest: {own.max():.3e} (list {int(np.argmax(own))})")
    value_bar = bars(name)["value"]
    means = {"mean L3": distance(out[1], m3), "mean L2": distance(out[2], m2)}
    print(f"[pose] {name:13s} means   hip vs float64: " + "  ".join(f"{k} {e:.3e}" for k, e in means.items()) + f"   bar: {value_bar:.3e}")
    over = np.nonzero(~(err <= bar))[0]
    problems = []
    if len(over):
        problems.append(f"{len(over)} of {len(lengths)} rows of lists off; worst: {where}, row {got[worst].tolist()} against {want[worst].tolist()}, "
                        f"{err[worst]:.3e} > {bar[worst]:.3e}; all (list, block, units, distance, bar): "
                        + str([(int(l), int(l) // 16, units[l], float(f"{err[l]:.3e}"), float(f"{bar[l]:.3e}")) for l in over]))
    if not (value_bar <= CAP and all(e <= value_bar for e in means.values())):
        problems.append(f"means off: {means}, bar {value_bar:.3e}")
    assert not problems, f"{name}: " + "; ".join(problems)
    assert out[3] == 0.0


@pytest.mark.gpu
def test_hip_pose_loss_first_and_last_pixel_of_a_wide_image():
    """200 x 328: ids above 2^16 and a width that is no power of two.  The gradients reach pixel 0 and pixel h * w - 1 of the first
    view (the case's first two matches name them) and are exactly zero at every pixel that no match names (dL/ddepth: of the pair's
    second view at every pixel - only the first view's depth is read)."""
    sc = scene("wide")
    h, w = sc.xyz.shape[-2:]
    a, c, _ = sc.corr[(0, 1)][0]
    _, got = run_hip("wide")
    d_xyz, d_depth = got["xyz"].reshape(2, 3, h * w).cpu(), got["depth"].reshape(2, h * w).cpu()
    for pixel in (0, h * w - 1):
        assert bool((d_xyz[0, :, pixel] != 0).all()) and bool((d_xyz[1, :, pixel] != 0).all()) and float(d_depth[0, pixel]) != 0, pixel
    named = torch.zeros(2, h * w, dtype=torch.bool)
    named[0, a], named[1, c] = True, True
    assert int(named[0].sum()) > 500 and not bool(d_xyz.permute(0, 2, 1)[~named].any())
    assert not bool(d_depth[0][~named[0]].any()) and not bool(d_depth[1].any())
    assert bool((d_xyz.permute(0, 2, 1)[named] != 0).any(-1).all()) and bool((d_depth[0][named[0]] != 0).all())


@pytest.mark.gpu
def test_hip_pose_loss_repeats_bit_for_bit():
    """The loss and dL/dposes of a repeated call are the same bits (fixed-order reductions), at every list count and list length
    (three blocks of lists, more than 64 lists, more than 64 units in a list); so are the gradients of a case in which no pixel
    receives more than two contributions."""
    for name in ("train42", "b7v5", "long"):
        (a, _, _), ga = run_hip(name)
        (b, _, _), gb = run_hip(name)
        assert torch.equal(a, b) and torch.equal(ga["poses"], gb["poses"]), name
    for name in ("v4", "v2"):
        (a, _, _), ga = run_hip(name)
        (b, _, _), gb = run_hip(name)
        assert torch.equal(a, b) and torch.equal(ga["poses"], gb["poses"]), name
    sc = scene("v2")  # one pair: a pixel gets more than one contribution only where ids repeat in a list
    ids = torch.cat([torch.cat([e[0], e[1] + H * W]) + 2 * H * W * s for s, e in enumerate(sc.corr[(0, 1)])])
    if int(torch.bincount(ids).max()) <= 2:
        assert torch.equal(ga["xyz"], gb["xyz"]) and torch.equal(ga["depth"], gb["depth"])


@pytest.mark.gpu
def test_hip_pose_loss_other_input_forms_give_the_same_bits():
    """Non-contiguous, float64 and (b, v, h, w)-shaped depth inputs are converted: the same bits as the plain form (the inputs are
    float32 numbers either way), and the gradients come back in the inputs' shapes and dtypes."""
    (plain, _, _), g0 = run_hip("b2v3")

    def strided(xyz, depth, poses, intr):
        wide = torch.zeros((*xyz.shape[:-1], 2 * W), device=xyz.device)
        wide[..., ::2] = xyz
        return wide[..., ::2], depth.reshape(2, 3, H, W).transpose(-1, -2).contiguous().transpose(-1, -2), poses.transpose(-1, -2).contiguous().transpose(-1, -2), intr

    forms = {"float64": lambda xyz, depth, poses, intr: (xyz.double(), depth.double(), poses.double(), intr.double()),
             "strided": strided, "depth (b, v, h, w)": lambda xyz, depth, poses, intr: (xyz, depth.reshape(2, 3, H, W), poses, intr)}
    for form, transform in forms.items():
        (value, _, _), g = run_hip("b2v3", transform=transform)
        assert torch.equal(value, plain), form
        assert torch.equal(g["poses"].float(), g0["poses"]), form
        assert g["depth"].shape == ((6, 1, H, W) if form == "float64" else (2, 3, H, W)) and g["xyz"].shape == g0["xyz"].shape
        assert g["xyz"].dtype == g["depth"].dtype == g["poses"].dtype == (torch.float64 if form == "float64" else torch.float32)
        for q in ("xyz", "depth"):  # float atomics: the same addends per pixel, a few of them, in another order - some float32 ulps (6e-8)
            assert distance(g[q].double().cpu().numpy().reshape(-1), g0[q].double().cpu().numpy().reshape(-1)) <= 1e-6, (form, q)


@pytest.mark.gpu
def test_losspose_module_takes_the_reference_structures_and_cotangents_scale():
    """Losspose.forward fed the reference's nested c2w / depth / corr equals pose_loss on the packed form, bit for bit; and
    (3 * loss).backward() gives three times the gradients (the cotangent is read on the device): three times the float64
    restatement's, within the case's bar."""
    from pf3plat_amd import losses

    (plain, _, _), g1 = run_hip("b2v3")
    _, g3 = run_hip("b2v3", scale=3.0)
    r64, bar = restated("b2v3", torch.float64), bars("b2v3")
    for q in ("xyz", "depth", "poses"):  # three times the float64 gradient, at the case's own bar
        got3, got1 = g3[q].double().cpu().numpy().reshape(r64[q].shape), g1[q].double().cpu().numpy().reshape(r64[q].shape)
        print(f"[pose] b2v3 x 3       {q:6s} hip vs 3 x float64: {distance(got3, 3 * r64[q]):.3e}   hip vs 3 x hip: {distance(got3, 3 * got1):.3e}   bar: {bar[q]:.3e}")
        assert distance(got3, 3 * r64[q]) <= bar[q], q
    sc = scene("b2v3")
    corr = {p: [tuple(t.to(DEV) for t in entry) for entry in lists] for p, lists in sc.corr.items()}
    conf = {p: c.to(DEV) for p, c in sc.conf.items()}
    poses = sc.poses.to(DEV).requires_grad_(True)
    module = losses.Losspose(losses.LossposeCfg(WEIGHT_2D, WEIGHT_3D))
    batch = {"target": {"intrinsics": sc.intrinsics.to(DEV)}}
    rel = torch.full((2, 3, 4, 4), float("nan"), device=DEV)  # c2w[0] is ignored
    value = module(None, batch, None, 0, (rel, poses), (sc.depth.to(DEV), None), (corr, None, conf), sc.xyz.to(DEV))
    assert torch.equal(value, plain)
    value.backward()
    assert torch.equal(poses.grad, g1["poses"])
