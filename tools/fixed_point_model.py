"""Which cotangent scales can a fixed-point accumulator serve?  A CPU model of the deterministic backward's sums (no GPU needed).

The deterministic backward (GSR_FLAG_DETERMINISTIC) adds every (tile, splat) contribution to a 64-bit integer sum after rounding it to
a fixed step (2^-32, gsr_hip.hip to_fixed).  The backward is linear in the cotangent image, so the contributions are obtained from the
fp64 oracle alone: one backward per 8 x 8 tile with the cotangent masked to that tile gives the per-(tile, splat) sums of dL/drgb,
dL/dopacity and dL/dmean2D at unit scale.  For a loss that is a mean (cotangent 2 N(0, delta) / count) they are scaled, rounded to the
step, summed over the tiles and compared with the exact sum: rel-L2 over the whole tensor, and the share of the non-zero
contributions that round to exactly 0.  With --unit the step is relative instead: the cotangents are first brought to units of the
image's largest |value| (a power of two: max 2^e in [1, 2)), which is what the library does per view.

A model, not a measurement: one contribution per (tile, splat); the constants the kernel folds into its first five slots (opacity,
half the image size, ln 2) are left out.  Scene: make_scene(31, 3000, (64, 64)), precomputed colours.  The table is in docs/PARITY.md, 8.

usage: python tools/fixed_point_model.py [--unit] [--step-bits 32]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd import synthetic  # noqa: E402
from pf3plat_amd.rasterizer import RasterConfig  # noqa: E402
from tests import gpu_util  # noqa: E402

N, HW = 3000, (64, 64)
ROWS = ((0.1, 3 * 64 * 64), (0.1, 3 * 3 * 256 * 256), (0.1, 4 * 3 * 3 * 256 * 256), (0.01, 3 * 3 * 256 * 256), (0.01, 64 * 3 * 3 * 256 * 256))
TENSORS = (("dL/drgb", "colors"), ("dL/dopacity", "opac"), ("dL/dmean2D", "means2d"))


def tile_contributions():
    """-> (unit cotangent (1, 3, H, W) fp64, {tensor: (tiles, ...) fp64 per-tile sums at unit scale})"""
    sc = synthetic.make_scene(31, N, HW)
    means, cov6, opac, colors = gpu_util.scene_tensors(sc, use_sh=False)
    vb = gpu_util.scene_viewbuf(sc)
    cfg = RasterConfig(1, 1, 1, N, *HW, 0, 0, 4, False)
    g = 2.0 * np.random.default_rng(31).normal(0.0, 1.0, (1, 3, *HW))
    parts = {k: [] for _, k in TENSORS}
    for ty in range(0, HW[0], 8):
        for tx in range(0, HW[1], 8):
            masked = np.zeros_like(g)
            masked[..., ty:ty + 8, tx:tx + 8] = g[..., ty:ty + 8, tx:tx + 8]
            o = gpu_util.run_oracle(cfg, vb, means, cov6, opac, colors, None, torch.tensor(masked), None, oracle_dtype=np.float64)
            for _, k in TENSORS:
                parts[k].append(np.asarray(o["grads"][k], np.float64))
    return g, {k: np.stack(v) for k, v in parts.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--unit", action="store_true", help="sums in units of the image's largest cotangent")
    ap.add_argument("--step-bits", type=int, default=32)
    a = ap.parse_args()
    g, parts = tile_contributions()
    step = 2.0 ** -a.step_bits
    print(f"| delta | count | {' | '.join(n for n, _ in TENSORS)} | contributions rounded to exactly 0 (rgb) |")
    print("|---|---|" + "---|" * (len(TENSORS) + 1))
    for delta, count in ROWS:
        f = delta / count
        unit = 2.0 ** -np.floor(np.log2(np.abs(g * f).max())) if a.unit else 1.0
        cells = []
        for _, k in TENSORS:
            c = parts[k] * (f * unit)
            fixed = np.clip(np.rint(c / step), -2.0 ** 62, 2.0 ** 62) * step
            exact, got = c.sum(0), fixed.sum(0)
            cells.append(f"{np.linalg.norm(got - exact) / np.linalg.norm(exact):.1e}")
        c = parts["colors"] * (f * unit)
        lost = float(((np.rint(c / step) == 0) & (c != 0)).sum() / max((c != 0).sum(), 1))
        print(f"| {delta} | {count} | {' | '.join(cells)} | {100 * lost:.0f} % |")


if __name__ == "__main__":
    main()
