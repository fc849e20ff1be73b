"""Writes tests/golden/attention_fixtures.npz (records self_rot, self_plain) and tests/golden/attention_fixtures_cross.npz (record
cross) by running the reference's OWN SelfBlock / CrossBlock / LearnableFourierPositionalEncoding on the CPU in float32.
usage: python tests/golden/make_attention_fixtures.py <PF3plat checkout>
lightglue.py is loaded by file path: the package's __init__ pulls in extractors that are not needed, the file alone imports with torch
and numpy.  The inputs and cotangents are the seeded ones of tests/attention_ref.record_inputs and are not stored; everything the
reference computed is: the state dict, the outputs, the gradients of inputs and parameters, and - from hooks on inner_attn, or on
to_qk, to_v and the input of to_out - q, k, v and the context, so the records serve at kernel level and at module level.  Two files:
the three records together would pass 1 MiB."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import attention_ref as ref  # noqa: E402

SHARPEN = 4.0  # Wqkv / to_qk times this: the softmax is not flat (the mean row maximum is printed)


def load_lightglue(checkout):
    path = os.path.join(checkout, "src", "model", "LightGlue", "lightglue", "lightglue.py")
    spec = importlib.util.spec_from_file_location("reference_lightglue", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def heads_first(t, heads):
    return t.unflatten(-1, (heads, -1)).transpose(1, 2)


def row_max(q, k, scale):
    return float(ref.probabilities(q.detach(), k.detach(), scale)[1].max(-1).values.mean())


def self_record(lg, name):
    _, _, E, H, B, N, _, with_enc, seed = ref.RECORDS[name]
    torch.manual_seed(seed)
    block = lg.SelfBlock(E, H, False)
    with torch.no_grad():
        block.Wqkv.weight.mul_(SHARPEN)
    inp = ref.record_inputs(name)
    x = inp["x"].clone().requires_grad_(True)
    enc = None
    if with_enc:
        posenc = lg.LearnableFourierPositionalEncoding(2, E // H, E // H)
        enc = posenc(inp["positions"]).detach().clone().requires_grad_(True)
    seen = {}
    block.inner_attn.register_forward_hook(lambda m, args, out: seen.update(q=args[0], k=args[1], v=args[2], context=out))
    out = block(x, enc)
    params = dict(block.named_parameters())
    wrt = [x] + ([enc] if enc is not None else []) + list(params.values())
    grads = torch.autograd.grad(out, wrt, inp["cot"])
    rec = {"out": out, "dx": grads[0], **seen}
    if enc is not None:
        rec["encoding"], rec["denc"] = enc, grads[1]
    rec.update({"state." + k: v for k, v in block.state_dict().items()})
    rec.update({"grad." + k: g for k, g in zip(params, grads[len(wrt) - len(params):])})
    print(f"{name}: mean row maximum of p {row_max(seen['q'], seen['k'], None):.3f}")
    return rec


def cross_record(lg, name):
    _, _, E, H, B, N, M, _, seed = ref.RECORDS[name]
    torch.manual_seed(seed)
    block = lg.CrossBlock(E, H, False)
    with torch.no_grad():
        block.to_qk.weight.mul_(SHARPEN)
    inp = ref.record_inputs(name)
    x0, x1 = inp["x0"].clone().requires_grad_(True), inp["x1"].clone().requires_grad_(True)
    qk, v, m = [], [], []
    block.to_qk.register_forward_hook(lambda mod, args, out: qk.append(heads_first(out, H)))
    block.to_v.register_forward_hook(lambda mod, args, out: v.append(heads_first(out, H)))
    block.to_out.register_forward_pre_hook(lambda mod, args: m.append(heads_first(args[0], H)))
    o0, o1 = block(x0, x1)
    params = dict(block.named_parameters())
    grads = torch.autograd.grad([o0, o1], [x0, x1] + list(params.values()), [inp["cot0"], inp["cot1"]])
    rec = {"out0": o0, "out1": o1, "dx0": grads[0], "dx1": grads[1], "qk0": qk[0], "qk1": qk[1], "v0": v[0], "v1": v[1], "m0": m[0], "m1": m[1]}
    rec.update({"state." + k: t for k, t in block.state_dict().items()})
    rec.update({"grad." + k: g for k, g in zip(params, grads[2:])})
    print(f"{name}: mean row maximum of p {row_max(qk[0], qk[1], block.scale):.3f} (m0), {row_max(qk[1], qk[0], block.scale):.3f} (m1)")
    return rec


def main():
    lg = load_lightglue(sys.argv[1])
    files = {}
    for name, spec in ref.RECORDS.items():
        rec = self_record(lg, name) if spec[1] == "self" else cross_record(lg, name)
        files.setdefault(spec[0], {}).update({f"{name}.{k}": np.ascontiguousarray(t.detach().numpy(), dtype=np.float32) for k, t in rec.items()})
    for fname, arrays in files.items():
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrays)
        print(f"{path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
