"""The yardstick of tests/test_lpips.py: the distance head of lpips.LPIPS(net="vgg"), version 0.1, eval mode, as include/gsr.h
defines it, restated in torch with a dtype switch - float64 the reference, float32 what the package itself runs -, the gradient in
closed form with the operator's zero-vector rule, the package's plain lines for autograd (`upstream_head`), the whole pipeline
(scaling layer, VGG16 features, head) for the module tests, the case table with its seeded generators, and the bars (docs/PARITY.md
section 23).  The package is not installed on any machine the suite runs on and is not part of the reference tree: the definition
in include/gsr.h is what both sides are held to.

Bars: every compared tensor (values, per-layer values, each layer's dL/da and dL/db) lies within
max(FLOOR, 4 x rel-L2(float32 restatement, float64 restatement)) rel-L2 of the float64 restatement, and no bar is above CAP.
FLOOR: the worst rel-L2 loss of the float32 restatement over every compared tensor of every case but the STRUCTURAL ones, measured
on the CPU the cases were fixed on; the CPU test checks its order of magnitude on the machine it runs on.

STRUCTURAL: the one gradient whose float32 restatement cannot come under CAP / 4 for ANY seed, because the definition's own
float32 arithmetic cancels there.  The rule (4 x the float32 restatement's loss) gives it a bar above CAP, which the tests state
instead of hiding; the device's error there is held to min(bar, CAP) = CAP, so no asserted bound is above the cap:
  "near", dL/da and dL/db: a^_c and b^_c are each rounded to 6e-8 relative and differ by 1e-3 relative, so every element of u - and
      with it of the gradient - carries 4e-5 relative in float32 (measured 4.27e-5 on either side; the VALUE averages that away:
      1.2e-6).  Bar 1.7e-4.
The gradient is evaluated in its projection form (`head_grad`), in float32 too: in the form the definition is written in, C = 1
gives noise (a float32 loss of 5.7: the two terms agree to ten digits); in the projection form the loss there is 2e-8."""
import functools

import torch
import torch.nn.functional as F

CAP = 1e-4
FLOOR = 1.2e-6  # measured: the worst float32 rel-L2 loss over the cases, structural tensors aside (1.18e-6, the values of "near")
STRUCTURAL = {("near", "da0"): 4.27e-5, ("near", "db0"): 4.27e-5}  # their measured float32 losses
EPS = 1e-10
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
VGG_CHANNELS = (64, 128, 256, 512, 512)
VGG_SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
NEAR = 1e-3

# name: (seed, n, ((C, h, w) per layer), kind).  Kinds: "relu" - relu(3 N(0, 1)) on either side, about half zeros; "zeros" - that,
# with all-zero vectors planted in a only, in b only and in both, and image 1 of a all zero; "near" - b = a (1 + 1e-3 N(0, 1));
# "far" - relu(N(0, 1)) x 10^U(-6, 4) per element.  "run+1": one pixel past two of the kernel's runs at C = 64 (the CPU test reads the
# run from the library and checks that).
_CHANNEL_EDGES = (1, 5, 63, 64, 65, 192, 512, 1024)
_PIXEL_EDGES = ((1, 1), (1, 77), (16, 16), (33, 31))
CASES = {
    **{f"c{c}": (100 + c, 2, ((c, 7, 9),), "relu") for c in _CHANNEL_EDGES},
    **{f"p{h}x{w}": (200 + h * w, 2, ((64, h, w),), "relu") for h, w in _PIXEL_EDGES},
    "run+1": (301, 2, ((64, 1, 2 * 256 + 1),), "relu"),
    "pyramid": (302, 3, tuple((c, 32 >> l, 32 >> l) for l, c in enumerate(VGG_CHANNELS)), "relu"),
    "one_layer": (303, 2, ((128, 6, 5),), "relu"),
    "two_layers": (304, 2, ((64, 12, 10), (128, 6, 5)), "relu"),
    "zeros": (305, 3, ((64, 9, 7), (192, 5, 4)), "zeros"),
    "near": (306, 2, ((512, 7, 9),), "near"),
    "far": (307, 2, ((65, 7, 9),), "far"),
    # the finish pass past its first trips: a wave takes the images n, n + 4, ..., a lane the units k, k + 64, ... of an image's layer
    "n9": (308, 9, ((64, 5, 7), (128, 3, 4)), "relu"),   # wave 0: images 0, 4 and 8
    "u65": (309, 2, ((512, 33, 63),), "relu"),           # runs of 32 pixels: 65 units an image, lane 0 alone takes a second
    "u129": (310, 2, ((512, 50, 82),), "relu"),          # 129 units an image: a third trip of one lane
    "u65c64": (311, 5, ((64, 129, 129),), "relu"),       # runs of 256: 66 units an image, and a fifth image for wave 0
}
FINISH_CASES = {"n9": (9, (1, 1)), "u65": (2, (65,)), "u129": (2, (129,)), "u65c64": (5, (66,))}  # name: (images, units an image per layer)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    den = float(b.norm())
    return float((a - b).norm()) / den if den > 0 else float((a - b).norm())


@functools.lru_cache(maxsize=None)
def make_case(name):
    """-> dict: fa, fb (lists of float32 (n, C, h, w)), ws (list of (C,)), g (n,), planted (per layer three bool (n, h, w) masks:
    zero in a only, in b only, in both).  float32 tensors; the float64 restatement reads their exact values."""
    seed, n, layers, kind = CASES[name]
    gen = torch.Generator().manual_seed(seed)
    fa, fb, ws, planted = [], [], [], []
    for C, h, w in layers:
        if kind == "far":
            a = F.relu(torch.randn((n, C, h, w), generator=gen)) * 10.0 ** (torch.rand((n, C, h, w), generator=gen) * 10 - 6)
            b = F.relu(torch.randn((n, C, h, w), generator=gen)) * 10.0 ** (torch.rand((n, C, h, w), generator=gen) * 10 - 6)
        else:
            a = F.relu(3 * torch.randn((n, C, h, w), generator=gen))
            b = a * (1 + NEAR * torch.randn((n, C, h, w), generator=gen)) if kind == "near" else F.relu(3 * torch.randn((n, C, h, w), generator=gen))
        za = zb = zab = torch.zeros((n, h, w), dtype=torch.bool)
        if kind == "zeros":
            pick = torch.rand((n, h, w), generator=gen)
            za, zb, zab = pick < 0.1, (pick >= 0.1) & (pick < 0.2), (pick >= 0.2) & (pick < 0.3)
            a_zero, b_zero = za | zab, zb | zab
            a_zero[1] = True  # a whole all-zero image on side a
            za, zb, zab = a_zero & ~b_zero, b_zero & ~a_zero, a_zero & b_zero
            a = a * (~(za | zab)).unsqueeze(1)
            b = b * (~(zb | zab)).unsqueeze(1)
        fa.append(a.float().contiguous())
        fb.append(b.float().contiguous())
        ws.append(torch.rand(C, generator=gen))
        planted.append((za, zb, zab))
    g = 0.5 + torch.rand(n, generator=gen)
    return {"fa": fa, "fb": fb, "ws": ws, "g": g, "planted": planted}


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def normalise(x):
    r = torch.sqrt(torch.sum(x * x, dim=1, keepdim=True))
    return x / (r + EPS), r


def head(fa, fb, ws, dtype):
    """-> (values (n,), per_layer (n, 5)) in `dtype`."""
    n = fa[0].shape[0]
    per_layer = torch.zeros((n, 5), dtype=dtype)
    for l, (a, b, w) in enumerate(zip(fa, fb, ws)):
        ah, _ = normalise(a.to(dtype))
        bh, _ = normalise(b.to(dtype))
        d = (ah - bh) ** 2 * w.to(dtype).view(1, -1, 1, 1)
        per_layer[:, l] = d.sum(dim=1).mean(dim=(1, 2))
    values = per_layer[:, 0].clone()
    for l in range(1, len(fa)):
        values = values + per_layer[:, l]
    return values, per_layer


def head_grad(fa, fb, ws, g, dtype):
    """The gradient in closed form (include/gsr.h), with the operator's rule: an all-zero vector's gradient is 0.
    -> (list of dL/da, list of dL/db) in `dtype`."""
    das, dbs = [], []
    for a, b, w in zip(fa, fb, ws):
        a, b, w = a.to(dtype), b.to(dtype), w.to(dtype).view(1, -1, 1, 1)
        hw = a.shape[2] * a.shape[3]
        ah, ra = normalise(a)
        bh, rb = normalise(b)
        na, nb = ra + EPS, rb + EPS
        u = 2 * g.to(dtype).view(-1, 1, 1, 1) * w * (ah - bh) / hw
        # in the projection form: with t = a / r_a and r_a / n_a = 1 - eps / n_a,
        #   u / n_a - a s / (r_a n_a^2) = (u - t q) / n_a + t q eps / n_a^2,  q = sum_c u_c t_c
        # (the two terms on the left agree to eps / n_a when u is parallel to a - always at C = 1 -, which float32 does not resolve)
        one = torch.ones_like(ra)
        ta, tb = a / torch.where(ra > 0, ra, one), b / torch.where(rb > 0, rb, one)
        qa = (u * ta).sum(dim=1, keepdim=True)
        qb = (-u * tb).sum(dim=1, keepdim=True)
        da = (u - ta * qa) / na + ta * qa * (EPS / na) / na
        db = (-u - tb * qb) / nb + tb * qb * (EPS / nb) / nb
        das.append(torch.where(ra > 0, da, torch.zeros_like(da)))
        dbs.append(torch.where(rb > 0, db, torch.zeros_like(db)))
    return das, dbs


def upstream_head(fa, fb, ws):
    """The package's own lines on feature maps (normalize_tensor, the squared difference, the `lin` 1 x 1 convolution without bias,
    spatial_average, the sum over the layers), in the tensors' dtype, for autograd."""
    val = 0
    for a, b, w in zip(fa, fb, ws):
        ah = a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + EPS)
        bh = b / (torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True)) + EPS)
        diff = (ah - bh) ** 2
        val = val + F.conv2d(diff, w.to(diff.dtype).view(1, -1, 1, 1)).mean([2, 3], keepdim=True)
    return val


def restatement(name, dtype):
    """-> dict of values, per_layer, da (list), db (list) for the case in `dtype`."""
    c = make_case(name)
    values, per_layer = head(c["fa"], c["fb"], c["ws"], dtype)
    da, db = head_grad(c["fa"], c["fb"], c["ws"], c["g"], dtype)
    return {"values": values, "per_layer": per_layer, "da": da, "db": db}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 restatement, float32 restatement) of a case: computed once and shared, never modified."""
    return restatement(name, torch.float64), restatement(name, torch.float32)


def compared(result):
    """The tensors a result is compared by, with their names."""
    out = [("values", result["values"]), ("per_layer", result["per_layer"])]
    out += [(f"da{l}", t) for l, t in enumerate(result["da"])] + [(f"db{l}", t) for l, t in enumerate(result["db"])]
    return out


def bars(name):
    r64, r32 = reference(name)
    return {key: max(FLOOR, 4.0 * rel_l2(t32, t64)) for (key, t64), (_, t32) in zip(compared(r64), compared(r32))}


def float32_losses(name):
    r64, r32 = reference(name)
    return {key: rel_l2(t32, t64) for (key, t64), (_, t32) in zip(compared(r64), compared(r32))}


# ---- the whole pipeline, for the module tests -----------------------------------------------------------------------------------------
def vgg_features(buffers, x, dtype):
    """buffers: the module's (conv{i}_weight / conv{i}_bias, shift, scale) on the CPU; x in [-1, 1] -> the five taps in `dtype`."""
    x = (x.to(dtype) - buffers["shift"].to(dtype)) / buffers["scale"].to(dtype)
    taps = []
    for k, s in enumerate(VGG_SLICES):
        if k > 0:
            x = F.max_pool2d(x, kernel_size=2, stride=2)
        for i in s:
            x = F.relu(F.conv2d(x, buffers[f"conv{i}_weight"].to(dtype), buffers[f"conv{i}_bias"].to(dtype), padding=1))
        taps.append(x)
    return taps


def pipeline(buffers, in0, in1, dtype, normalize=False):
    """LPIPS.forward restated with the package's lines (autograd carries the gradient) -> (n, 1, 1, 1) in `dtype`."""
    in0, in1 = in0.to(dtype), in1.to(dtype)
    if normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    ws = [buffers[f"lin{k}"] for k in range(5)]
    return upstream_head(vgg_features(buffers, in0, dtype), vgg_features(buffers, in1, dtype), ws)


def term_scale(name, side):
    """The float64 norm of the first term of the gradient, u / n_a (side "a") or u / n_b (side "b"), per layer: the size of what the
    gradient is formed from (the STRUCTURAL note above)."""
    c = make_case(name)
    out = []
    for a, b, w in zip(c["fa"], c["fb"], c["ws"]):
        a, b, w = a.double(), b.double(), w.double().view(1, -1, 1, 1)
        ah, ra = normalise(a)
        bh, rb = normalise(b)
        u = 2 * c["g"].double().view(-1, 1, 1, 1) * w * (ah - bh) / (a.shape[2] * a.shape[3])
        out.append(float((u / ((ra if side == "a" else rb) + EPS)).norm()))
    return out
