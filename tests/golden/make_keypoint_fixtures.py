"""Writes tests/golden/keypoint_fixtures.npz by running the reference's OWN simple_nms, top_k_keypoints and sample_descriptors on the
CPU in float32.
usage: python tests/golden/make_keypoint_fixtures.py <PF3plat checkout>
superpoint.py is loaded by file path inside a stub package: its two imports that the three functions do not use - kornia.color's
rgb_to_grayscale and the package's .utils (Extractor) - are stub modules.  The reference's SuperPoint class is never constructed (its
__init__ fetches weights).  The inputs are the seeded ones of tests/keypoint_ref.py and are not stored; what the reference made is:
the bit-packed keep masks (simple_nms(s, r) > 0) of the score cases and of the three staircase batches, one sample_descriptors output
and one top_k_keypoints result."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import keypoint_ref as ref  # noqa: E402


def load_superpoint(checkout):
    path = os.path.join(checkout, "src", "model", "LightGlue", "lightglue", "superpoint.py")
    kornia, color = types.ModuleType("kornia"), types.ModuleType("kornia.color")
    color.rgb_to_grayscale = None
    kornia.color = color
    package, utils = types.ModuleType("reference_lightglue"), types.ModuleType("reference_lightglue.utils")
    package.__path__ = []
    utils.Extractor = torch.nn.Module
    sys.modules.update({"kornia": kornia, "kornia.color": color, "reference_lightglue": package, "reference_lightglue.utils": utils})
    spec = importlib.util.spec_from_file_location("reference_lightglue.superpoint", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pack(mask):
    return np.packbits(mask.numpy().astype(np.uint8).reshape(-1))


def main():
    sp = load_superpoint(sys.argv[1])
    arrays = {}
    with torch.no_grad():
        for name, (_, _, _, _, _, r) in ref.SCORE_CASES.items():
            kept = sp.simple_nms(ref.score_case(name), r) > 0
            arrays["nms." + name] = pack(kept)
            print(f"{name}: {int(kept.sum())} kept of {kept.numel()}")
        for direction in "hvd":
            s, want = ref.staircase(direction)
            kept = sp.simple_nms(s, 4) > 0
            arrays["stairs." + direction] = pack(kept)
            for b, pts in enumerate(want):  # what the issue states, on the reference's own function
                assert sorted((int(x), int(y)) for y, x in zip(*torch.where(kept[b]))) == sorted(pts), (direction, b)
        seven = torch.zeros(1, 12, 64)
        seven[0, 5, 3:31:4] = torch.arange(10.0, 3.0, -1.0)
        arrays["stairs.seven"] = torch.where(sp.simple_nms(seven, 4)[0, 5] > 0)[0].numpy()  # (the seventh stair is never kept)
        pix, desc = ref.sample_inputs()
        dense = torch.nn.functional.normalize(desc, p=2, dim=1)
        arrays["sample"] = sp.sample_descriptors(pix[None].float(), dense, 8)[0].T.contiguous().numpy()
        scores, k = ref.topk_inputs()
        kp = torch.arange(scores.numel())
        top, top_scores = sp.top_k_keypoints(kp, scores, k)
        arrays["topk"] = top.numpy()
    np.savez_compressed(ref.FIXTURES, **arrays)
    print(f"{ref.FIXTURES}: {len(arrays)} arrays, {os.path.getsize(ref.FIXTURES)} bytes")
    assert os.path.getsize(ref.FIXTURES) < 1_000_000


if __name__ == "__main__":
    main()
