"""Writes tests/golden/match_fixtures.npz by running the reference's OWN MatchAssignment and filter_matches on the CPU in float32.
usage: python tests/golden/make_match_fixtures.py <PF3plat checkout>
lightglue.py is loaded by file path, as make_attention_fixtures.py loads it.  The descriptors are the seeded ones of
tests/match_ref.record_inputs and are not stored; what the reference made is: the module's state dict (final_proj's weight
sharpened, so that the softmaxes are not flat) and matches0 / 1, matching_scores0 / 1 at filter threshold 0.1."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import match_ref as ref  # noqa: E402


def load_lightglue(checkout):
    path = os.path.join(checkout, "src", "model", "LightGlue", "lightglue", "lightglue.py")
    spec = importlib.util.spec_from_file_location("reference_lightglue", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    lg = load_lightglue(sys.argv[1])
    arrays = {}
    for name, (B, m, n, d, seed) in ref.RECORDS.items():
        torch.manual_seed(seed)
        module = lg.MatchAssignment(d)
        with torch.no_grad():
            module.final_proj.weight.mul_(ref.RECORD_SHARPEN)
            desc0, desc1 = ref.record_inputs(name)
            scores, _ = module(desc0, desc1)
            m0, m1, ms0, ms1 = lg.filter_matches(scores, ref.THRESHOLD)
        rec = {"matches0": m0, "matches1": m1, "matching_scores0": ms0, "matching_scores1": ms1}
        rec.update({"state." + k: v for k, v in module.state_dict().items()})
        arrays.update({f"{name}.{k}": np.ascontiguousarray(t.detach().numpy()) for k, t in rec.items()})
        print(f"{name}: {int((m0 > -1).sum())} matches of {B} x {m}, mean row maximum of the assignment {float(scores[:, :-1, :-1].max(2).values.exp().mean()):.3f}")
    path = ref.FIXTURES
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
