"""The yardstick of tests/test_keypoints.py: SuperPoint.forward's lines after its last two convolutions
(src/model/LightGlue/lightglue/superpoint.py:52-95, 171-227, with the rescale of utils.py:146) restated in torch with a dtype switch
- float64 the reference, float32 what the reference itself runs -, the seeded inputs of the records in
tests/golden/keypoint_fixtures.npz (made by the reference's own simple_nms, top_k_keypoints and sample_descriptors:
tests/golden/make_keypoint_fixtures.py), the case tables and the bars (docs/PARITY.md section 22).

From the scores on every decision is a comparison: the scores form is judged EXACTLY on every case, ties included.  The logits form is
judged exactly too, which is fair only where no decision lies within rounding: `conditions` measures, in float64, for every max-pool
window the restatement evaluates on scores (maxpool(s) and the two maxpool(supp_scores)) the relative distance of its two highest
DISTINCT values - equal values are both zero or a planted tie, equal logits within one cell, which are bit-equal on any
implementation - and the relative distance of every candidate's score from the threshold; the CPU test asserts both >= GAP for every
case (seeds chosen so).

SCORE_LOSS: the largest relative |float32 restatement - float64 restatement| of a score over the cases; GAP = 100 x that.  FLOOR_*:
the worst rel-L2 loss of the float32 restatement over the cases.  All measured on the CPU the fixtures were made on; the CPU test
checks their order of magnitude on the machine it runs on."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "golden", "keypoint_fixtures.npz")
TILE = 32            # pf3plat_amd.keypoints.TILE, which the CPU test holds this to: the cases place their edges by it
CAP = 1e-4           # no bar is above this
SCORE_LOSS = 1.2e-6  # measured: the largest relative |float32 - float64| of a score over the cases (1.16e-6, case "batch")
GAP = 100 * SCORE_LOSS
FLOOR_SCORES = 4.1e-7       # measured: the worst float32 rel-L2 loss of the keypoint scores over the cases (4.03e-7, case "s2x3")
FLOOR_DESCRIPTORS = 6.6e-7  # measured: ... of the descriptors (6.51e-7, case "batch")
THRESHOLD = 0.0005
DEFAULTS = dict(nms_radius=4, detection_threshold=THRESHOLD, remove_borders=4, max_num_keypoints=None)

# ---- the logits form: name: (seed, B, h, w in cells, C, kind, parameters other than the defaults, scales or None) ------------------
# kinds: "plain"; "ties": equal logits planted inside cells; "dustbin": image 1 of the batch has no keypoint
T8 = TILE // 8
LOGIT_CASES = {
    "s1x1": (1, 1, 1, 1, 8, "plain", {}, None),
    "s2x3": (2, 1, 2, 3, 8, "plain", {}, None),
    "s3x3": (3, 2, 3, 3, 8, "plain", {}, None),
    "s9x17": (4, 1, 9, 17, 256, "plain", {}, None),
    "tm8": (5, 1, T8 - 1, T8, 8, "plain", {}, None),
    "tp8": (6, 1, T8, T8 + 1, 8, "plain", {}, None),
    "t2p8": (7, 1, 2 * T8 + 1, T8 - 1, 8, "plain", {}, None),
    "w2p8": (8, 1, T8 + 1, 2 * T8 + 1, 8, "ties", {}, None),
    "batch": (1035, 3, 16, 16, 32, "dustbin", {}, ((1.0, 1.0), (0.5, 0.75), (1.6, 1.25))),
    "r0": (10, 1, 5, 6, 8, "plain", {"nms_radius": 0, "detection_threshold": 0.02}, None),
    "r2": (11, 1, 5, 6, 8, "plain", {"nms_radius": 2}, None),
    "th0": (12, 1, 5, 6, 8, "plain", {"detection_threshold": 0.0}, None),
    "b0": (13, 2, 5, 6, 16, "plain", {"remove_borders": 0}, ((2.0, 0.8), (0.7, 1.3))),
    "c1": (14, 1, 5, 6, 1, "plain", {}, None),
    "c5": (15, 1, 5, 6, 5, "plain", {}, None),
    "c64": (16, 1, 5, 6, 64, "plain", {}, None),
    "c255": (17, 1, 5, 6, 255, "plain", {}, None),
    "c256": (18, 1, 5, 6, 256, "plain", {"remove_borders": 0}, None),
    "topk": (119, 2, 6, 6, 8, "ties", {}, None),
}
# ---- the scores form: name: (seed, B, H, W in pixels, kind, nms_radius) - every one recorded from the reference's simple_nms --------
# kinds: "uniform": continuous; "eighths": multiples of 1 / 8 (many ties, zeros among them)
SCORE_CASES = {
    "u37x61": (31, 2, 37, 61, "uniform", 4),
    "q37x61": (32, 2, 37, 61, "eighths", 4),
    "q67x29": (33, 1, 2 * TILE + 3, TILE - 3, "eighths", 4),
    "q33x95": (34, 1, TILE + 1, 3 * TILE - 1, "eighths", 2),
    "q40x40r0": (35, 1, 40, 40, "eighths", 0),
    "u24x72": (36, 1, TILE - 8, 2 * TILE + 8, "uniform", 4),
    "q32x64": (37, 1, TILE, 2 * TILE, "eighths", 4),
}
# ---- the loops only large calls enter (scores form, judged exactly against `select`; no record of the reference is needed) ---------
SCAN_CHUNK = 2048    # mask words (32 pixels of a row each) a trip of the scan pass takes; it carries the keypoints counted so far
BASE_STEP = 256      # images a trip of an image's first packed row (the counts before it, summed by 256 threads) takes
TOPK_CHUNK = 8192    # found keypoints a trip of the top-k pass ranks against; it carries every keypoint's rank so far
# name: (seed, H, W, nms_radius, remove_borders), one image in eighths: H x ceil(W / 32) words
SCAN_CASES = {
    "w2048": (50, 1024, 40, 1, 0),   # 2048 words: one trip exactly
    "w2049": (51, 2049, 24, 1, 0),   # one word in the second trip
    "w2080": (51, 1040, 40, 2, 4),   # 2080 words, two a row
}
BATCH_CASE = (81, 260, 8, 8, 1, 0, 0.95, 2, 8)  # seed, B, H, W, nms_radius, remove_borders, threshold, max_num_keypoints of the cut, C
# name: (seed, H, W, found count, max_num_keypoints): eighths, nms_radius 0 and no border - every pixel above the threshold is found -,
# the last non-zero pixels zeroed until `found` are left
TOPK_CASES = {
    "k8192": (61, 100, 100, TOPK_CHUNK, 6000),       # one trip exactly
    "k8193": (62, 100, 100, TOPK_CHUNK + 1, 6000),   # a second trip of one keypoint
    "k3trips": (63, 140, 140, None, 12000),          # as drawn: more than two chunks
}
STAIR_OFFSETS = TILE + 25         # start offsets 0 ... TILE + 24
STAIR_EDGE = TILE + 24 + 20 + 12  # the long edge of a staircase image: the last stair of the last offset, and 11 pixels more
STAIR_THIN = 12                   # the short edge of the horizontal and vertical ones; the stairs lie on line 5
SAMPLE = (41, 40, 256, 9, 17)     # seed, keypoints, C, h, w: the sample_descriptors record
TOPK = (42, 50, 20)               # seed, n, k: the top_k_keypoints record


def rel_l2(a, b):
    a, b = a.double(), b.double()
    den = float(b.norm())
    return float((a - b).norm()) / den if den > 0 else float((a - b).norm())


def gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def logit_case(name):
    """(logits (B, 65, h, w), descriptors (B, C, h, w), scales (B, 2) or None, parameters), float32, seeded."""
    seed, B, h, w, C, kind, params, scales = LOGIT_CASES[name]
    g = gen(seed)
    logits = 2.5 * torch.randn(B, 65, h, w, generator=g)
    logits[:, 64] = 1.0 + torch.randn(B, h, w, generator=g)
    if kind == "ties":  # equal logits inside a cell: equal scores on any implementation; the cells around it quiet, so that they are maxima
        for b in range(B):
            for n, (i, j, chans) in enumerate(((1, 1, (9, 14, 63)), (h - 2, w - 2, (0, 36)), (h // 2, 1, (27, 28, 35)))):
                logits[b, 64, i - 1:i + 2, j - 1:j + 2] = 9.0
                logits[b, 64, i, j] = 0.0
                logits[b, :64, i, j].clamp_(max=3.0)
                logits[b, list(chans), i, j] = 6.0 + b + 0.5 * n
    if kind == "dustbin":
        logits[1, 64] = 22.0   # image 1: the dustbin dominates, every score below exp(-8)
        logits[2, 64] += 2.5   # image 2: fewer keypoints than image 0
    desc = torch.randn(B, C, h, w, generator=g) * (0.2 + 3.0 * torch.rand(B, 1, h, w, generator=g))
    p = dict(DEFAULTS)
    p.update(params)
    return logits, desc, None if scales is None else torch.tensor(scales, dtype=torch.float32), p


@functools.lru_cache(maxsize=None)
def score_case(name):
    seed, B, H, W, kind, r = SCORE_CASES[name]
    g = gen(seed)
    if kind == "uniform":
        return torch.rand(B, H, W, generator=g)
    return torch.randint(0, 9, (B, H, W), generator=g).float() / 8


def eighths(seed, *shape):
    return torch.randint(0, 9, shape, generator=gen(seed)).float() / 8


@functools.lru_cache(maxsize=None)
def scan_case(name):
    """(scores (1, H, W), parameters, what `select` finds) of a SCAN_CASES entry."""
    seed, H, W, r, border = SCAN_CASES[name]
    s = eighths(seed, 1, H, W)
    kw = dict(nms_radius=r, remove_borders=border)
    return s, kw, select(s, **kw)


def mask_words(pixels, W):
    """The index of each pixel's mask word in the image's row-major order of (row, word of the row)."""
    return pixels[:, 1] * ((W + 31) // 32) + pixels[:, 0] // 32


@functools.lru_cache(maxsize=None)
def batch_case():
    """(scores (B, H, W) uniform, descriptors (B, C, H / 8, W / 8), parameters) of BATCH_CASE."""
    seed, B, H, W, r, border, thr, _, C = BATCH_CASE
    g = gen(seed)
    s = torch.rand(B, H, W, generator=g)
    desc = torch.randn(B, C, H // 8, W // 8, generator=g)
    return s, desc, dict(nms_radius=r, remove_borders=border, detection_threshold=thr)


@functools.lru_cache(maxsize=None)
def topk_case(name):
    """(scores (1, H, W), parameters with the cut, what `select` finds and keeps, the found keypoints' scores in row-major order)."""
    seed, H, W, found, k = TOPK_CASES[name]
    s = eighths(seed, 1, H, W)
    if found is not None:
        flat = s.view(-1)
        flat[torch.nonzero(flat)[found:, 0]] = 0.0
    kw = dict(nms_radius=0, remove_borders=0, max_num_keypoints=k)
    staged = select(s, nms_radius=0, remove_borders=0)[0][1]
    return s, kw, select(s, **kw), staged


def chunk_ranks(scores, chunk=None):
    """The top-k pass's count, chunk by chunk: row c holds for every keypoint i the keypoints j of chunk c with a higher score, or an
    equal one and j < i.  The rows' sum is the keypoint's place in the stable descending sort."""
    chunk = TOPK_CHUNK if chunk is None else chunk
    n = scores.numel()
    idx = torch.arange(n)
    rows = []
    for c0 in range(0, n, chunk):
        part = scores[c0:c0 + chunk]
        up = torch.sort(part).values
        rk = part.numel() - torch.searchsorted(up, scores, right=True)  # the higher ones
        for v in part.unique():
            tie = part == v
            before = torch.cumsum(tie, 0) - tie.long()  # of the chunk's keypoints below j, those equal to v
            j = (idx - c0).clamp(0, part.numel())
            rk = rk + torch.where(scores == v, torch.cat([before, tie.sum()[None]])[j], torch.zeros_like(rk))
        rows.append(rk)
    return torch.stack(rows)


@functools.lru_cache(maxsize=None)
def staircase(direction):
    """(scores (2 STAIR_OFFSETS, H, W), expected pixels per image): image 2 o has the six stairs 10, 9, ... 5, spaced 4 apart along
    `direction` ("h", "v" or "d") from offset o, image 2 o + 1 the same without the first.  Expected: stairs 0, 2, 4 and 1, 3, 5."""
    dx, dy = {"h": (1, 0), "v": (0, 1), "d": (1, 1)}[direction]
    H = STAIR_EDGE if dy else STAIR_THIN
    W = STAIR_EDGE if dx else STAIR_THIN
    s = torch.zeros(2 * STAIR_OFFSETS, H, W)
    want = []
    for o in range(STAIR_OFFSETS):
        at = [((o + 4 * t) if dx else 5, (o + 4 * t) if dy else 5) for t in range(6)]
        for t, (x, y) in enumerate(at):
            s[2 * o, y, x] = 10.0 - t
            if t:
                s[2 * o + 1, y, x] = 10.0 - t
        want += [[at[0], at[2], at[4]], [at[1], at[3], at[5]]]
    return s, want


@functools.lru_cache(maxsize=None)
def sample_inputs():
    seed, n, C, h, w = SAMPLE
    g = gen(seed)
    desc = torch.randn(1, C, h, w, generator=g)
    pix = torch.stack([torch.randint(0, 8 * w, (n,), generator=g), torch.randint(0, 8 * h, (n,), generator=g)], -1)
    return pix, desc


@functools.lru_cache(maxsize=None)
def topk_inputs():
    seed, n, k = TOPK
    return torch.rand(n, generator=gen(seed)), k


@functools.lru_cache(maxsize=None)
def fixtures():
    with np.load(FIXTURES) as f:
        return {k: f[k] for k in f.files}


def unpack_mask(name, shape):
    bits = np.unpackbits(fixtures()[name])[: int(np.prod(shape))]
    return torch.from_numpy(bits.reshape(shape).astype(bool))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def scores_from_logits(logits, dtype):
    """Step 1: the softmax over the 65 channels, channel 64 dropped, cell (i, j)'s channel 8 a + c to pixel (8 i + a, 8 j + c)."""
    p = torch.softmax(logits.to(dtype), 1)[:, :64]
    B, _, h, w = p.shape
    return p.reshape(B, 8, 8, h, w).permute(0, 3, 1, 4, 2).reshape(B, 8 * h, 8 * w)


def max_pool(x, r):
    return F.max_pool2d(x[:, None], 2 * r + 1, 1, r)[:, 0]  # (pads with -inf)


def nms_mask(s, r, windows=None):
    """Step 2: simple_nms's max_mask (B, H, W) bool.  `windows`: a list that receives every score array a max-pool runs on."""
    note = windows.append if windows is not None else (lambda x: None)
    note(s)
    mask = s == max_pool(s, r)
    for _ in range(2):
        supp = max_pool(mask.to(s.dtype), r) > 0
        ss = torch.where(supp, torch.zeros_like(s), s)
        note(ss)
        mask = mask | ((ss == max_pool(ss, r)) & ~supp)
    return mask


def select(s, nms_radius=4, detection_threshold=THRESHOLD, remove_borders=4, max_num_keypoints=None, windows=None):
    """Steps 2 and 3 on scores (B, H, W): per image (pixels (n, 2) int64 (x, y), scores (n,), count found)."""
    B, H, W = s.shape
    keep = nms_mask(s, nms_radius, windows) & (s > detection_threshold)
    inner = torch.zeros(H, W, dtype=torch.bool, device=s.device)
    if H > 2 * remove_borders and W > 2 * remove_borders:
        inner[remove_borders:H - remove_borders, remove_borders:W - remove_borders] = True
    out = []
    for b in range(B):
        y, x = torch.where(keep[b] & inner)  # row-major
        sc = s[b][y, x]
        n = int(y.numel())
        if max_num_keypoints is not None and n > max_num_keypoints:
            order = torch.sort(sc, descending=True, stable=True).indices[:max_num_keypoints]  # ties: the lower row-major index first
            y, x, sc = y[order], x[order], sc[order]
        out.append((torch.stack([x, y], -1), sc, n))
    return out


def sample(pixels, desc, dtype):
    """Step 4: pixels (n, 2) (x, y), desc (C, h, w) NOT normalised -> (n, C)."""
    C, h, w = desc.shape
    d = desc.to(dtype)
    d = d / d.norm(dim=0, keepdim=True).clamp_min(1e-12)
    p = pixels.to(dtype)
    ix = (p[:, 0] - 3.5) / (8 * w - 4.5) * (w - 1)
    iy = (p[:, 1] - 3.5) / (8 * h - 4.5) * (h - 1)
    x0, y0 = ix.floor(), iy.floor()
    tx, ty = ix - x0, iy - y0
    out = torch.zeros(p.shape[0], C, dtype=dtype, device=d.device)
    for ox, oy, wt in ((0, 0, (1 - tx) * (1 - ty)), (1, 0, tx * (1 - ty)), (0, 1, (1 - tx) * ty), (1, 1, tx * ty)):
        xi, yi = (x0 + ox).long(), (y0 + oy).long()
        inb = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        col = d[:, yi.clamp(0, h - 1), xi.clamp(0, w - 1)].T * inb[:, None].to(dtype)
        out = out + wt[:, None] * col
    return out / out.norm(dim=1, keepdim=True).clamp_min(1e-12)


def rescale(pixels, scale, dtype):
    """Step 5: (pixel + 0.5) / scale - 0.5; scale (2,) or None."""
    p = pixels.to(dtype)
    return p if scale is None else (p + 0.5) / scale.to(dtype) - 0.5


def detect(logits, desc, scales, params, dtype, windows=None):
    """The whole chain: per image a dict of pixels, keypoints, keypoint_scores, descriptors, count."""
    s = scores_from_logits(logits, dtype)
    out = []
    for b, (pix, sc, n) in enumerate(select(s, windows=windows, **params)):
        out.append({"pixels": pix, "keypoint_scores": sc, "count": n, "descriptors": sample(pix, desc[b], dtype),
                    "keypoints": rescale(pix, None if scales is None else scales[b], dtype)})
    return out


def conditions(name):
    """In float64: (the smallest relative distance of the two highest distinct values of a max-pool window on scores, the smallest
    relative distance of a candidate's score from the threshold) of a logits case."""
    logits, desc, scales, p = logit_case(name)
    windows = []
    res = detect(logits, desc, scales, p, torch.float64, windows)
    r, gap = p["nms_radius"], float("inf")
    for x in windows:
        v = F.unfold(x[:, None], 2 * r + 1, padding=r)  # (zero padding: a zero second value is a distance of 1)
        top = v.max(1).values
        second = torch.where(v == top[:, None], torch.full_like(v, -1.0), v).max(1).values.clamp_min(0)
        live = top > 0
        if live.any():
            gap = min(gap, float(((top - second) / top.clamp_min(1e-300))[live].min()))
    thr = p["detection_threshold"]
    found = sum(r_["count"] for r_ in res)
    # (a candidate is what passed NMS inside the borders, whichever side of the threshold it is on)
    s = scores_from_logits(logits, torch.float64)
    q = dict(p, detection_threshold=-1.0, max_num_keypoints=None)
    cand = torch.cat([sc for _, sc, _ in select(s, **q)])
    near = float(((cand - thr).abs() / cand).min()) if thr > 0 and cand.numel() else float("inf")
    return gap, near, found


@functools.lru_cache(maxsize=None)
def logit_reference(name):
    """(float64 restatement, float32 restatement) of a logits case, computed once."""
    logits, desc, scales, p = logit_case(name)
    return detect(logits, desc, scales, p, torch.float64), detect(logits, desc, scales, p, torch.float32)


def score_loss(name):
    """The largest relative |float32 - float64| of a score of a logits case."""
    logits = logit_case(name)[0]
    s64, s32 = scores_from_logits(logits, torch.float64), scores_from_logits(logits, torch.float32)
    return float(((s32.double() - s64).abs() / s64).max())
