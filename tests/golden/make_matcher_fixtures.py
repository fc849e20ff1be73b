"""Writes tests/golden/matcher_fixtures.npz by running the reference's OWN LightGlue(features=None, depth_confidence=-1,
width_confidence=-1) on the CPU in float32 (features=None: nothing is fetched).
usage: python tests/golden/make_matcher_fixtures.py <PF3plat checkout>
lightglue.py is loaded by file path, as make_match_fixtures.py loads it.  The 12 M weights are NOT stored: tests/matcher_ref.seeded_state
makes every tensor from its name, its shape and a seed, and this script loads that into the reference's module (strict).  The inputs are
the seeded ones of tests/matcher_ref.record_inputs and are not stored either.  Stored per record: the names and shapes of the reference's
state dict (JSON), the descriptors after the last layer (a forward hook on the last TransformerLayer), matches0 / 1 and
matching_scores0 / 1."""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import matcher_ref as ref  # noqa: E402


def load_lightglue(checkout):
    path = os.path.join(checkout, "src", "model", "LightGlue", "lightglue", "lightglue.py")
    spec = importlib.util.spec_from_file_location("reference_lightglue", path)
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec.loader.exec_module(mod)
    return mod


def main():
    lg = load_lightglue(sys.argv[1])
    arrays = {}
    for name, (B, m, n, n_layers, wseed, _) in ref.RECORDS.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            module = lg.LightGlue(features=None, depth_confidence=-1, width_confidence=-1, n_layers=n_layers).eval()
        shapes = [(k, list(v.shape)) for k, v in module.state_dict().items()]
        module.load_state_dict(ref.seeded_state([(k, tuple(s)) for k, s in shapes], wseed), strict=True)
        seen = {}
        module.transformers[-1].register_forward_hook(lambda mod, args, out: seen.update(desc0=out[0], desc1=out[1]))
        desc0, desc1, kpts0, kpts1 = ref.record_inputs(name)
        size = torch.tensor([ref.SIZE] * B, dtype=torch.float32)
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = module({"image0": {"keypoints": kpts0, "descriptors": desc0, "image_size": size},
                          "image1": {"keypoints": kpts1, "descriptors": desc1, "image_size": size}})
        assert out["stop"] == n_layers
        rec = {"desc0": seen["desc0"], "desc1": seen["desc1"], "matches0": out["matches0"], "matches1": out["matches1"],
               "matching_scores0": out["matching_scores0"], "matching_scores1": out["matching_scores1"]}
        arrays[f"{name}.names_and_shapes"] = np.array(json.dumps(shapes))
        arrays.update({f"{name}.{k}": np.ascontiguousarray(t.detach().numpy()) for k, t in rec.items()})
        print(f"{name}: {int((out['matches0'] > -1).sum())} matches of {B} x {m}, {sum(int(np.prod(s)) for _, s in shapes)} parameters not stored")
    np.savez_compressed(ref.FIXTURES, **arrays)
    print(f"{ref.FIXTURES}: {len(arrays)} arrays, {os.path.getsize(ref.FIXTURES)} bytes")
    assert os.path.getsize(ref.FIXTURES) < 1_000_000


if __name__ == "__main__":
    main()
