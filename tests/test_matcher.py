"""LightGlue's transformer on the device (pf3plat_amd.matcher): the restatement of tests/matcher_ref.py against the records of the
reference's own LightGlue (CPU), the module's state dict, refusals and checks (CPU), and TransformerLayer / LightGlue / the
pair_lists -> LightGlue -> pack_matched chain against the records and the float64 restatement (GPU); one layer on 34 lists - 68
units in either attention, past a trip of the ragged attention's unit search (docs/PARITY.md section 24.1)."""
import functools

import pytest
import torch

from pf3plat_amd import _lib, matcher, matching
from pf3plat_amd.keypoints import PackedKeypoints
from tests import matcher_ref as ref

gpu = pytest.mark.gpu
BAR = 4.0 * ref.MODULE_LOSS  # the final descriptors of the HIP path against the float64 restatement: 4 x the float32 restatement's own loss


def _all_calls():
    """(label, float64 result, float32 result) of every list-by-list call the bars are measured on."""
    for name in ref.RECORDS:
        yield name, ref.record_restatement(name, torch.float64), ref.record_restatement(name, torch.float32)
    for i, (a, b) in enumerate(zip(ref.ragged_restatement(torch.float64), ref.ragged_restatement(torch.float32))):
        yield f"ragged{i}", a, b
    for i, (a, b) in enumerate(zip(ref.chain_restatement(torch.float64), ref.chain_restatement(torch.float32))):
        yield f"chain{i}", a, b


MANY_SEED, MANY_LAYER = 91, 3


@functools.lru_cache(maxsize=None)
def many_lists():
    """34 lists, 68 units in either attention of a layer - the unit search of the ragged attention takes 64 a trip -: sides of 1 to 20
    keypoints, list 5 (140, 3) - a side of two query blocks in the first trip -, list 20 and list 31 with an empty side, list 33
    (2, 131) - two query blocks in the second trip of the self-attention, image 1 of the last list, and of the cross-attention."""
    g = torch.Generator().manual_seed(MANY_SEED)
    sides = torch.randint(1, 21, (34, 2), generator=g).tolist()
    sides[5], sides[20], sides[31], sides[33] = [140, 3], [9, 0], [0, 7], [2, 131]
    return tuple((m, n) for m, n in sides)


@functools.lru_cache(maxsize=None)
def many_layer(dtype=torch.float64):
    """Layer MANY_LAYER of rec9 on each of the 34 lists in `dtype`, list by list: (x0', x1'), or None where a side is empty (the
    reference passes such a list through no layer)."""
    lists = ref.inputs(many_lists(), MANY_SEED)
    return [ref.layer(ref.state_of("rec9"), MANY_LAYER, *(t[None] for t in l), dtype) if m and n else None
            for l, (m, n) in zip(lists, many_lists())]


def _layer_calls():
    """(label, float64 result, float32 result) of the one-layer calls on the 34 lists: the descriptors alone."""
    for l, (a, b) in enumerate(zip(many_layer(torch.float64), many_layer(torch.float32))):
        if a is not None:
            yield f"many{l}", {"desc0": a[0], "desc1": a[1]}, {"desc0": b[0], "desc1": b[1]}


# ---- CPU
def test_many_lists_take_the_unit_search_of_both_attentions_past_its_first_trip():
    sizes = many_lists()
    lay = matcher.list_layout([m for m, _ in sizes], [n for _, n in sizes])
    step, rows = 64, sum(m + n for m, n in sizes)
    print(f"{len(sizes)} lists, {rows} rows, {len(lay.self_ranges)} units in either attention")
    assert len(sizes) > 32 and len(lay.self_ranges) == len(lay.cross_q) == len(lay.cross_k) == 2 * len(sizes) > step and 900 <= rows <= 1100
    assert sum(1 for m, n in sizes if m == 0 or n == 0) == 2 and (140, 3) in sizes[:32] and sizes[-1] == (2, 131)
    assert all(1 <= s <= 20 for l, mn in enumerate(sizes) if l not in (5, 20, 31, 33) for s in mn)
    for ranges in (lay.self_ranges, lay.cross_q):
        blocks = [(c + 127) // 128 for _, c in ranges]
        assert sum(blocks[:step]) not in (0, step)       # what the search carries into its second trip is not the unit count
        assert blocks[-1] == 2 and sum(blocks[step:]) >= 4  # ... and there it finds a unit of two blocks behind others
    # a search without the carry would pair unit u >= 64 with the keys of unit u - 64: other lists' rows
    assert all(lay.cross_k[u] != lay.cross_k[u - step] and lay.self_ranges[u] != lay.self_ranges[u - step] for u in range(step, 2 * len(sizes)))
    worst = max(ref.rel_l2(r32[key], r64[key]) for _, r64, r32 in _layer_calls() for key in ("desc0", "desc1"))
    print(f"one layer on the 34 lists: worst float32 loss {worst:.3e}, bar {BAR:.3e}")
    assert 4.0 * worst <= BAR


def test_module_floor_is_the_worst_float32_loss():
    worst, worst_max0 = 0.0, 0.0
    for label, r64, r32 in _layer_calls():
        worst = max(worst, ref.rel_l2(r32["desc0"], r64["desc0"]), ref.rel_l2(r32["desc1"], r64["desc1"]))
    for label, r64, r32 in _all_calls():
        for key in ("desc0", "desc1"):
            if r64[key].numel():
                worst = max(worst, ref.rel_l2(r32[key], r64[key]))
        if r64["max0"].numel():
            worst_max0 = max(worst_max0, float((r32["max0"].double() - r64["max0"]).abs().max()))
    print(f"worst float32 loss of the final descriptors {worst:.3e}, of max0 {worst_max0:.3e}")
    assert worst <= ref.MODULE_LOSS <= 2.0 * worst
    assert worst_max0 <= ref.MAX0_LOSS <= 2.0 * worst_max0
    assert BAR <= 1e-4  # the project's cap


def test_every_match_is_decided_by_more_than_the_gap():
    """In float64 every top-two gap and every distance from the threshold is at least GAP = 100 x the float32 loss of max0: the
    matches of these inputs are judged exactly, no row is left out, and the float32 restatement alone agrees with the float64 one."""
    for label, r64, r32 in _all_calls():
        keep0, keep1 = ref.exact_rows(r64)
        assert bool(keep0.all()) and bool(keep1.all()), (label, int((~keep0).sum()), int((~keep1).sum()))
        assert torch.equal(r32["matches0"], r64["matches0"]) and torch.equal(r32["matches1"], r64["matches1"]), label


@pytest.mark.parametrize("name", list(ref.RECORDS))
def test_restatement_reproduces_the_references_records(name):
    rec, r64, r32 = ref.record(name), ref.record_restatement(name), ref.record_restatement(name, torch.float32)
    for key in ("desc0", "desc1"):
        err = ref.rel_l2(rec[key], r64[key])
        print(name, key, f"reference against float64 {err:.3e}, against float32 {ref.rel_l2(rec[key], r32[key]):.3e}")
        assert err <= 2.0 * ref.MODULE_LOSS  # the reference's own float32 arithmetic (SDPA) against float64
    assert torch.equal(rec["matches0"], r64["matches0"]) and torch.equal(rec["matches1"], r64["matches1"])
    for key in ("matching_scores0", "matching_scores1"):
        assert float((rec[key].double() - r64[key]).abs().max()) <= 2.0 * ref.MAX0_LOSS  # (d exp(x) <= dx: scores are at most 1)


def _module(name):
    m = matcher.LightGlue(n_layers=ref.RECORDS[name][3])
    m.load_state_dict(ref.state_of(name), strict=True)
    return m.eval()


@pytest.mark.parametrize("name", list(ref.RECORDS))
def test_state_dict_is_the_references(name):
    m = matcher.LightGlue(n_layers=ref.RECORDS[name][3])
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == ref.names_and_shapes(name)
    m.load_state_dict(ref.state_of(name), strict=True)
    assert not any(p.requires_grad and p.grad is not None for p in m.parameters())


def test_refused_configurations_raise():
    for kw in (dict(depth_confidence=0.95), dict(width_confidence=0.99), dict(add_scale_ori=True), dict(n_layers=0)):
        with pytest.raises(ValueError, match="LightGlue"):
            matcher.LightGlue(**kw)
    with pytest.raises(ValueError, match="TransformerLayer"):
        matcher.TransformerLayer(256, 2)  # 128 channels per head
    with pytest.raises(ValueError, match="TransformerLayer"):
        matcher.TransformerLayer(250, 4)
    m = matcher.LightGlue(input_dim=128, n_layers=1)
    assert isinstance(m.input_proj, torch.nn.Linear) and len(m.token_confidence) == 0 and len(m.log_assignment) == 1


def test_python_checks_fire_before_the_library_loads(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))
    m = matcher.LightGlue(n_layers=1)
    d, k = torch.zeros(5, 256), torch.zeros(5, 2)
    with pytest.raises(ValueError, match="size"):
        m(d, d, k, k, [5], [5], None)
    with pytest.raises(ValueError, match="LightGlue"):
        m(d, d, k, k, [5], None, ref.SIZE)
    with pytest.raises(ValueError, match="LightGlue"):
        m(d, d, k, k, [4], [5], ref.SIZE)
    with pytest.raises(ValueError, match="LightGlue"):
        m(d, d, k, k, [5], [5, 0], ref.SIZE)
    with pytest.raises(ValueError, match="LightGlue"):
        m(d, d[:, :8], k, k, [5], [5], ref.SIZE)
    with pytest.raises(ValueError, match="LightGlue"):
        m(d, d, k, k, None, None, ref.SIZE)  # (the equal-length form is (B, m, d))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(d, d, k, k, [5], [5], ref.SIZE)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(d[None], d[None], k[None], k[None], size=ref.SIZE)
    packed = PackedKeypoints(torch.zeros(9, 2), torch.zeros(9, 2, dtype=torch.int32), torch.zeros(9), torch.zeros(9, 256), (3, 3, 3))
    with pytest.raises(ValueError, match="pair_lists"):
        matcher.pair_lists(packed, 2, 3)
    with pytest.raises(ValueError, match="pair_lists"):
        matcher.pair_lists(packed._replace(descriptors=None), 1, 3)


def test_pair_lists_order_is_pack_matcheds():
    """list l = pair x num_scenes + scene, pairs (0, 1), (0, 2), (1, 2), images in (b v) order: plain indexing, no GPU."""
    desc, kpts, counts = ref.chain_inputs()
    packed = PackedKeypoints(kpts, kpts.to(torch.int32), torch.zeros(len(kpts)), desc, counts)
    lists = matcher.pair_lists(packed, 2, 3)
    want = ref.chain_lists()
    assert lists.lengths0 == tuple(len(l[0]) for l in want) and lists.lengths1 == tuple(len(l[1]) for l in want)
    assert torch.equal(lists.desc0, torch.cat([l[0] for l in want])) and torch.equal(lists.desc1, torch.cat([l[1] for l in want]))
    assert torch.equal(lists.kpts0, torch.cat([l[2] for l in want])) and torch.equal(lists.kpts1, torch.cat([l[3] for l in want]))


def test_list_layout():
    lay = matcher.list_layout((3, 0, 2), (4, 5, 0))
    assert lay.self_ranges == ((0, 3), (3, 0), (3, 2), (5, 4), (9, 5), (14, 0))
    assert lay.cross_q == ((0, 3), (5, 4), (3, 0), (9, 5), (3, 2), (14, 0))
    assert lay.cross_k == ((5, 4), (0, 3), (9, 5), (3, 0), (14, 0), (3, 2))


# ---- GPU
def _judge(label, m0, m1, s0, s1, r64):
    """One list's dense outputs against the float64 restatement: matches exactly, scores within the float32 loss of max0."""
    assert torch.equal(m0.cpu(), r64["matches0"][0]) and torch.equal(m1.cpu(), r64["matches1"][0]), label
    for got, key in ((s0, "matching_scores0"), (s1, "matching_scores1")):
        if got.numel():
            assert float((got.cpu().double() - r64[key][0]).abs().max()) <= 4.0 * ref.MAX0_LOSS, (label, key)


@gpu
@pytest.mark.parametrize("name", list(ref.RECORDS))
def test_lightglue_reproduces_the_records(name):
    """The equal-length (B, m, .) form against the reference's own record and the float64 restatement."""
    B, m, n = ref.RECORDS[name][:3]
    module = _module(name).cuda()
    desc0, desc1, kpts0, kpts1 = (t.cuda() for t in ref.record_inputs(name))
    x, layout = module.encode(desc0, desc1, kpts0, kpts1, None, None, ref.SIZE)
    res = module(desc0, desc1, kpts0, kpts1, size=ref.SIZE)
    rec, r64 = ref.record(name), ref.record_restatement(name)
    got0, got1 = x[:B * m].reshape(B, m, -1), x[B * m:].reshape(B, n, -1)
    for got, key in ((got0, "desc0"), (got1, "desc1")):
        err = ref.rel_l2(got, r64[key])
        print(name, key, f"{err:.3e} against float64, {ref.rel_l2(got, rec[key]):.3e} against the record; bar {BAR:.3e}")
        assert err <= BAR
    assert res.matches0.shape == (B, m) and res.matches1.shape == (B, n)
    assert torch.equal(res.matches0.cpu(), rec["matches0"]) and torch.equal(res.matches1.cpu(), rec["matches1"])
    assert torch.equal(res.matches0.cpu(), r64["matches0"]) and torch.equal(res.matches1.cpu(), r64["matches1"])
    for key in ("matching_scores0", "matching_scores1"):
        assert float((getattr(res, key).cpu().double() - r64[key]).abs().max()) <= 4.0 * ref.MAX0_LOSS


@gpu
def test_transformer_layer_on_the_ragged_lists():
    """One layer (rec9's fourth) on the six-list packed buffer against the float64 restatement list by list."""
    module = _module("rec9").cuda()
    lists = ref.inputs(ref.RAGGED, ref.RAGGED_SEED)
    lay = matcher.list_layout([m for m, _ in ref.RAGGED], [n for _, n in ref.RAGGED])
    x = torch.cat([l[0] for l in lists] + [l[1] for l in lists]).cuda()
    kpts = torch.cat([l[2] for l in lists] + [l[3] for l in lists]).cuda()
    rot = module.posenc(matcher.normalize_keypoints(kpts, ref.SIZE))[:, 0].contiguous()
    out = module.transformers[3](x, rot, lay)
    assert out.shape == x.shape
    M0 = lay.offsets0[-1]
    worst = 0.0
    for l, (m, n) in enumerate(ref.RAGGED):
        if m == 0 or n == 0:
            continue  # (the reference passes such a list through no layer; nothing reads what the device made of it)
        w0, w1 = ref.layer(ref.state_of("rec9"), 3, *(t[None] for t in lists[l]))
        got0, got1 = out[lay.offsets0[l]:lay.offsets0[l + 1]], out[M0 + lay.offsets1[l]:M0 + lay.offsets1[l + 1]]
        worst = max(worst, ref.rel_l2(got0, w0[0]), ref.rel_l2(got1, w1[0]))
    print(f"one layer: {worst:.3e}, bar {BAR:.3e}")
    assert worst <= BAR and not bool(torch.isnan(out).any())


@gpu
def test_transformer_layer_on_34_lists():
    """One layer (rec9's fourth) on 34 lists - 68 units in either attention, more than a trip of the unit search - against the float64
    restatement list by list; twice: the same bits."""
    module = _module("rec9").cuda()
    sizes = many_lists()
    lists = ref.inputs(sizes, MANY_SEED)
    lay = matcher.list_layout([m for m, _ in sizes], [n for _, n in sizes])
    x = torch.cat([l[0] for l in lists] + [l[1] for l in lists]).cuda()
    kpts = torch.cat([l[2] for l in lists] + [l[3] for l in lists]).cuda()
    rot = module.posenc(matcher.normalize_keypoints(kpts, ref.SIZE))[:, 0].contiguous()
    out = module.transformers[MANY_LAYER](x, rot, lay)
    assert out.shape == x.shape and not bool(torch.isnan(out).any())
    M0 = lay.offsets0[-1]
    worst, at = 0.0, None
    for l, want in enumerate(many_layer()):
        if want is None:
            continue
        got0, got1 = out[lay.offsets0[l]:lay.offsets0[l + 1]], out[M0 + lay.offsets1[l]:M0 + lay.offsets1[l + 1]]
        for err in (ref.rel_l2(got0, want[0][0]), ref.rel_l2(got1, want[1][0])):
            assert err <= BAR, (l, sizes[l], err, BAR)  # (every list by itself: a short list does not hide behind a long one)
            worst, at = (err, l) if err > worst else (worst, at)
    print(f"one layer on 34 lists: worst {worst:.3e} (list {at}, {sizes[at]}), bar {BAR:.3e}")
    assert torch.equal(module.transformers[MANY_LAYER](x, rot, lay), out)


@gpu
def test_lightglue_on_the_ragged_lists():
    module = _module("rec9").cuda()
    lists = ref.inputs(ref.RAGGED, ref.RAGGED_SEED)
    len0, len1 = [m for m, _ in ref.RAGGED], [n for _, n in ref.RAGGED]
    args = [torch.cat([l[i] for l in lists]).cuda() for i in range(4)]
    x, lay = module.encode(*args, len0, len1, ref.SIZE)
    res = module(*args, len0, len1, ref.SIZE, width=ref.SIZE[0])
    again = module(*args, len0, len1, ref.SIZE, width=ref.SIZE[0])
    assert torch.equal(res.matches0, again.matches0) and torch.equal(res.matching_scores0, again.matching_scores0)  # the same bits
    want, M0, worst = ref.ragged_restatement(), lay.offsets0[-1], 0.0
    found = res.lists()
    for l, (m, n) in enumerate(ref.RAGGED):
        o0, o1, r64 = lay.offsets0[l], lay.offsets1[l], want[l]
        _judge(f"list {l}", res.matches0[o0:o0 + m], res.matches1[o1:o1 + n], res.matching_scores0[o0:o0 + m], res.matching_scores1[o1:o1 + n], r64)
        assert torch.equal(found[l][0].cpu(), r64["matches"][0])
        if m and n:
            worst = max(worst, ref.rel_l2(x[o0:o0 + m], r64["desc0"][0]), ref.rel_l2(x[M0 + o1:M0 + o1 + n], r64["desc1"][0]))
        else:
            assert int((res.matches0[o0:o0 + m] > -1).sum()) == 0 and len(found[l][0]) == 0
    print(f"six lists, final descriptors: {worst:.3e}, bar {BAR:.3e}")
    assert worst <= BAR


@gpu
def test_chain_from_packed_keypoints_to_packed_correspondences():
    """pair_lists -> LightGlue -> pack_matched for 2 scenes x 3 views gives the lists of the restatement run pair by pair."""
    module = _module("rec9").cuda()
    desc, kpts, counts = ref.chain_inputs()
    packed = PackedKeypoints(kpts.cuda(), kpts.to(torch.int32).cuda(), torch.zeros(len(kpts)).cuda(), desc.cuda(), counts)
    lists = matcher.pair_lists(packed, 2, 3)
    res = module(lists.desc0, lists.desc1, lists.kpts0, lists.kpts1, lists.lengths0, lists.lengths1, ref.SIZE, width=ref.SIZE[0])
    corr, points = matching.pack_matched(res, 2)
    want, inputs = ref.chain_restatement(), ref.chain_lists()
    assert len(corr.offsets) == 7 and corr.offsets[-1] == len(points)
    for l, r64 in enumerate(want):
        pairs = r64["matches"][0]
        a, b = corr.offsets[l], corr.offsets[l + 1]
        assert b - a == len(pairs), l
        k0, k1 = inputs[l][2][pairs[:, 0]], inputs[l][3][pairs[:, 1]]
        assert torch.equal(corr.ids_i[a:b].cpu(), k0[:, 1].long() * ref.SIZE[0] + k0[:, 0].long())
        assert torch.equal(corr.ids_j[a:b].cpu(), k1[:, 1].long() * ref.SIZE[0] + k1[:, 0].long())
        assert torch.equal(points[a:b].cpu(), k0)
    assert sum(len(r["matches"][0]) for r in want) > 100  # (the chain carries matches: 4 of the 6 lists have both sides)
