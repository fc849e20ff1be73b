"""The yardstick of the matcher tests: LightGlue._forward without pruning or early stop (reference
src/model/LightGlue/lightglue/lightglue.py:25-36, 61-74, 133-247, 477-597) restated on the blocks of tests/attention_ref.py and the
assignment of tests/match_ref.py, with a dtype switch - float64 is the reference, float32 measures what the reference's own arithmetic
loses -, run LIST BY LIST as the reference runs it; the seeded weights and inputs, and the records of the reference's own LightGlue
(tests/golden/make_matcher_fixtures.py).  CPU only."""
import functools
import json
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests import attention_ref, match_ref
from tests.attention_ref import rel_l2  # noqa: F401

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matcher_fixtures.npz")
DIM, HEADS, SIZE, THRESHOLD = 256, 4, (640, 480), 0.1
RESIDUAL = 0.3  # the last linear of every FFN: the residual stream keeps its scale over nine layers, and the similarity stays moderate
SHARPEN = 3.0  # final_proj's weight, as tests/match_ref.RECORD_SHARPEN: the softmaxes of the assignment are not flat
# name: (B, m, n, n_layers, seed of the weights, seed of the inputs)
RECORDS = {"rec9": (2, 70, 150, 9, 31, 41), "rec2": (1, 45, 33, 2, 32, 42)}
# The ragged six-list call of the GPU tests: (m, n) per list, 1203 rows; its weights are rec9's, its inputs seeded by RAGGED_SEED.
RAGGED = ((70, 150), (45, 0), (1, 77), (131, 323), (0, 33), (333, 40))
RAGGED_SEED = 78  # (the first of a search from 43 on at which no row of the six lists lies within GAP of a tie or of the threshold)
CHAIN_SEED = 49  # the pair_lists chain: 2 scenes x 3 views
CHAIN_COUNTS = (150, 70, 131, 97, 0, 160)  # keypoints of the six images, (b v) order

# What the float32 restatement loses against the float64 one on the FINAL DESCRIPTORS (rel-L2; measured on the CPU by
# tests/test_matcher.py::test_module_floor_is_the_worst_float32_loss, which prints it; rounded up in the second digit), at worst over
# the two records and the ragged call: the module-level bar of the GPU tests is 4 x this, for the different summation order.
MODULE_LOSS = 4.0e-7
# ... and the largest |float32 - float64| of max0 (the log of a row's best assignment score) over the same calls; GAP = 100 x that.
MAX0_LOSS = 1.7e-4
GAP = 100 * MAX0_LOSS
GAP_SHARE = 0.02  # the share of a list's rows that may lie within GAP of a tie or of the threshold and are then left out


def seeded_state(names_and_shapes, seed):
    """Every tensor of a LightGlue state dict from its name, its shape and a seed: linear weights normal with variance 1 / fan-in
    (final_proj's sharpened, an FFN's last one times RESIDUAL), LayerNorm weights around 1, biases small, the encoding's Wr normal.  float32."""
    state = {}
    for name, shape in names_and_shapes:
        g = torch.Generator().manual_seed((zlib.crc32(name.encode()) + 7919 * seed) % (2 ** 31))
        t = torch.randn(*shape, generator=g, dtype=torch.float64)
        if name == "confidence_thresholds":
            t = torch.rand(*shape, generator=g, dtype=torch.float64)
        elif name.endswith("posenc.Wr.weight"):
            pass
        elif name.endswith(".weight") and len(shape) == 2:
            t = t / shape[1] ** 0.5
            if name.endswith("final_proj.weight"):
                t = t * SHARPEN
            if name.endswith("ffn.3.weight"):
                t = t * RESIDUAL
        elif name.endswith(".weight"):
            t = 1.0 + 0.1 * t
        else:
            t = 0.05 * t
        state[name] = t.to(torch.float32)
    return state


def inputs(lists, seed):
    """Planted descriptors (tests/match_ref.planted_descriptors) and keypoints inside SIZE for (m, n) lists: per list desc0 (m, DIM),
    desc1 (n, DIM), kpts0 (m, 2), kpts1 (n, 2), float32."""
    g = torch.Generator().manual_seed(seed)
    out = []
    wh = torch.tensor(SIZE, dtype=torch.float32)
    for m, n in lists:
        x0, x1 = match_ref.planted_descriptors(g, m, n, DIM)
        out.append((x0, x1, torch.rand(m, 2, generator=g) * (wh - 1), torch.rand(n, 2, generator=g) * (wh - 1)))
    return out


def _sub(state, prefix):
    return {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}


def encoding(state, kpts, dtype):
    """normalize_keypoints with a given size, then LearnableFourierPositionalEncoding.forward: (2, B, 1, n, head_dim)."""
    size = torch.tensor(SIZE, dtype=dtype)
    k = (kpts.to(dtype) - (size / 2)) / (size.max() / 2)
    projected = F.linear(k, state["posenc.Wr.weight"])
    return torch.stack([torch.cos(projected), torch.sin(projected)], 0).unsqueeze(-3).repeat_interleave(2, dim=-1)


def lightglue(state, n_layers, desc0, desc1, kpts0, kpts1, dtype=torch.float64):
    """LightGlue._forward for equal-length lists desc0 (B, m, DIM), desc1 (B, n, DIM): the final descriptors and what
    tests/match_ref.assignment makes of the last layer's head."""
    st = {k: v.to(dtype) for k, v in state.items()}
    x0, x1 = desc0.to(dtype), desc1.to(dtype)
    if "input_proj.weight" in st:
        x0, x1 = (F.linear(x, st["input_proj.weight"], st["input_proj.bias"]) for x in (x0, x1))
    if x0.shape[1] > 0 and x1.shape[1] > 0:  # (lightglue.py:533: a list with an empty side passes no layer)
        e0, e1 = encoding(st, kpts0, dtype), encoding(st, kpts1, dtype)
        for i in range(n_layers):
            s, c = _sub(st, f"transformers.{i}.self_attn."), _sub(st, f"transformers.{i}.cross_attn.")
            x0 = attention_ref.self_block(s, HEADS, x0, e0)[0]
            x1 = attention_ref.self_block(s, HEADS, x1, e1)[0]
            x0, x1 = attention_ref.cross_block(c, HEADS, x0, x1)[0]
    head = _sub(st, f"log_assignment.{n_layers - 1}.")
    md0, md1 = (F.linear(x, head["final_proj.weight"], head["final_proj.bias"]) for x in (x0, x1))
    z0, z1 = (F.linear(x, head["matchability.weight"], head["matchability.bias"]) for x in (x0, x1))
    res = match_ref.assignment(md0, md1, z0, z1, THRESHOLD, dtype)
    res.update(desc0=x0, desc1=x1, mdesc0=md0, mdesc1=md1, z0=z0, z1=z1)
    return res


def layer(state, index, x0, x1, kpts0, kpts1, dtype=torch.float64):
    """One TransformerLayer of the state on one list: (x0', x1')."""
    st = {k: v.to(dtype) for k, v in state.items()}
    e0, e1 = encoding(st, kpts0, dtype), encoding(st, kpts1, dtype)
    s, c = _sub(st, f"transformers.{index}.self_attn."), _sub(st, f"transformers.{index}.cross_attn.")
    x0 = attention_ref.self_block(s, HEADS, x0.to(dtype), e0)[0]
    x1 = attention_ref.self_block(s, HEADS, x1.to(dtype), e1)[0]
    return attention_ref.cross_block(c, HEADS, x0, x1)[0]


@functools.lru_cache(maxsize=None)
def fixtures():
    with np.load(FIXTURES) as f:
        return {k: f[k] for k in f.files}


def names_and_shapes(name):
    return [(n, tuple(s)) for n, s in json.loads(str(fixtures()[name + ".names_and_shapes"]))]


@functools.lru_cache(maxsize=None)
def state_of(name):
    return seeded_state(names_and_shapes(name), RECORDS[name][4])


def record_inputs(name):
    B, m, n, _, _, seed = RECORDS[name]
    lists = inputs(((m, n),) * B, seed)
    return tuple(torch.stack([l[i] for l in lists]) for i in range(4))  # desc0 (B, m, DIM), desc1, kpts0, kpts1


@functools.lru_cache(maxsize=None)
def record(name):
    return {k[len(name) + 1:]: torch.from_numpy(v) for k, v in fixtures().items() if k.startswith(name + ".") and v.dtype.kind in "fi"}


@functools.lru_cache(maxsize=None)
def record_restatement(name, dtype=torch.float64):
    return lightglue(state_of(name), RECORDS[name][3], *record_inputs(name), dtype)


@functools.lru_cache(maxsize=None)
def ragged_restatement(dtype=torch.float64):
    """The six-list call, list by list, at rec9's weights: a list of `lightglue` results."""
    state, n_layers = state_of("rec9"), RECORDS["rec9"][3]
    return [lightglue(state, n_layers, *(t[None] for t in l), dtype) for l in inputs(RAGGED, RAGGED_SEED)]


def exact_rows(res64, gap=None):
    """Per list of a float64 result: the rows of image 0 whose match is decided by more than `gap` - the top-two gap of the row's and
    of its best column's arg-maximum, and the distance of the score's log from log(threshold)."""
    gap = GAP if gap is None else gap
    md0, md1, z0, z1 = res64["mdesc0"], res64["mdesc1"], res64["z0"], res64["z1"]
    B, m, d = md0.shape
    n = md1.shape[1]
    keep, keep1 = torch.ones(B, m, dtype=torch.bool), torch.ones(B, n, dtype=torch.bool)
    if m == 0 or n == 0:
        return keep, keep1
    for b in range(B):
        s = (md0[b] / d ** 0.25) @ (md1[b] / d ** 0.25).T
        lr, lc = torch.logsumexp(s, 1), torch.logsumexp(s, 0)
        a = 2 * s - lc[None] + F.logsigmoid(z1[b].reshape(1, n))
        bb = 2 * s - lr[:, None] + F.logsigmoid(z0[b].reshape(m, 1))
        row_gap = torch.full((m,), float("inf"), dtype=s.dtype)
        if n >= 2:
            top = a.topk(2, 1).values
            row_gap = top[:, 0] - top[:, 1]
        col_gap = torch.full((n,), float("inf"), dtype=s.dtype)
        if m >= 2:
            top = bb.topk(2, 0).values
            col_gap = top[0] - top[1]
        best = a.argmax(1)
        near_threshold = (res64["max0"][b] - float(np.log(THRESHOLD))).abs()
        keep[b] = (row_gap > gap) & (col_gap[best] > gap) & (near_threshold > gap)
        keep1[b] = (col_gap > gap) & keep[b][bb.argmax(0)]  # a column is decided when its best row is
    return keep, keep1


def chain_inputs(seed=None):
    """The packed keypoints of 2 scenes x 3 views, (b v) order: per image, noisy copies of a random part of its scene's pool of 200
    descriptors (so every pair of a scene shares partners) and keypoints inside SIZE.  -> descriptors (sum, DIM), keypoints (sum, 2), counts."""
    g = torch.Generator().manual_seed(CHAIN_SEED if seed is None else seed)
    wh = torch.tensor(SIZE, dtype=torch.float32)
    desc, kpts = [], []
    for image, count in enumerate(CHAIN_COUNTS):
        if image % 3 == 0:
            pool = torch.randn(200, DIM, generator=g)
        rows = torch.randperm(200, generator=g)[:count]
        desc.append(pool[rows] + 0.1 * torch.randn(count, DIM, generator=g))
        kpts.append(torch.rand(count, 2, generator=g) * (wh - 1))
    return torch.cat(desc), torch.cat(kpts), CHAIN_COUNTS


def chain_lists(seed=None):
    """... and its (pair, scene) lists in the order pack_matched expects, list = pair x 2 + scene: (desc0, desc1, kpts0, kpts1) each."""
    desc, kpts, counts = chain_inputs(seed)
    starts = [0]
    for c in counts:
        starts.append(starts[-1] + c)
    cut = lambda t, image: t[starts[image]:starts[image + 1]]
    return [(cut(desc, 3 * s + a), cut(desc, 3 * s + b), cut(kpts, 3 * s + a), cut(kpts, 3 * s + b))
            for a, b in ((0, 1), (0, 2), (1, 2)) for s in range(2)]


@functools.lru_cache(maxsize=None)
def chain_restatement(dtype=torch.float64):
    state, n_layers = state_of("rec9"), RECORDS["rec9"][3]
    return [lightglue(state, n_layers, *(t[None] for t in l), dtype) for l in chain_lists()]
