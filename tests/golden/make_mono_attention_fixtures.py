"""Generates tests/golden/mono_attention_fixtures.npz by RUNNING the reference's own module on the CPU:
`DepthPredictorMultiView.forward` (src/model/encoder/costvolume/depth_predictor_multiview.py) up to the input of
`depth_head_lowres`, with `UNetModel` - the one import that module does not need here - stubbed by a subclass of nn.Identity.
`multi_reg` is zeroed and `gamma` set to 1, so `fused_cost_volume` IS `multi_out` (line 367; the interpolation of line 371 is to the
same size).  Forward hooks on the three 1 x 1 convolutions capture q, k and v (lines 360, 361, 365: the convolutions' outputs before
the `.view`), a pre-hook on `depth_head_lowres` captures its input and stops the forward; autograd then gives the gradients of that
input with respect to the three captured tensors for a seeded cotangent.  The weights of lin_mono_q / lin_mono_k are scaled to widen
the scores.  Per record: q, k (n, E, L) and v (n, C, L) as the `.view` lays them out, the output, the cotangent and the three
gradients, float32.

    python tests/golden/make_mono_attention_fixtures.py <path of a PF3plat checkout>
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
from torch import nn

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "mono_attention_fixtures.npz")
# name: (seed, b, v, h, w, D, feature channels, weight scale)
RECORDS = {"record_a": (21, 1, 2, 8, 12, 128, 8, 300.0), "record_b": (22, 2, 2, 16, 12, 32, 4, 40.0)}


class _Stop(Exception):
    pass


class _IdentityUNet(nn.Identity):
    pass


def import_reference(root):
    for name, path in [("src", "src"), ("src.model", "src/model"), ("src.model.encoder", "src/model/encoder"),
                       ("src.model.encoder.costvolume", "src/model/encoder/costvolume"),
                       ("src.model.encoder.costvolume.ldm_unet", "src/model/encoder/costvolume/ldm_unet")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(root, path)]
        sys.modules[name] = m
    unet = types.ModuleType("src.model.encoder.costvolume.ldm_unet.unet")
    unet.UNetModel = _IdentityUNet
    sys.modules[unet.__name__] = unet
    return importlib.import_module("src.model.encoder.costvolume.depth_predictor_multiview")


def run_record(mod, seed, b, v, h, w, D, c, scale):
    from tests import cost_volume_ref

    torch.manual_seed(seed)
    net = mod.DepthPredictorMultiView(feature_channels=c, num_depth_candidates=D, costvolume_unet_feat_dim=8, gaussian_raw_channels=4,
                                      depth_unet_feat_dim=4, num_views=v)
    with torch.no_grad():
        for p in net.multi_reg.parameters():
            p.zero_()
        net.gamma.fill_(1.0)
        net.lin_mono_q.weight.mul_(scale)
        net.lin_mono_k.weight.mul_(scale)
    got = {}
    hooks = [getattr(net, name).register_forward_hook(lambda _m, _i, o, key=key: got.__setitem__(key, o))
             for key, name in (("q", "lin_mono_q"), ("k", "lin_mono_k"), ("v", "lin_multi_v"))]

    def stop(_m, args):
        got["out"] = args[0]
        raise _Stop

    hooks.append(net.depth_head_lowres.register_forward_pre_hook(stop))
    case = cost_volume_ref.build_case(seed, b, v, c, h, w, D, 0.05)
    g = torch.Generator().manual_seed(seed)
    cue = torch.nn.functional.one_hot(torch.randint(0, D, (v * b, h, w), generator=g), D).permute(0, 3, 1, 2).float().contiguous()
    try:
        net(case["features"], case["intrinsics"], case["extrinsics"], case["near"], case["far"], extra_info={"monocular_cue": cue})
    except _Stop:
        pass
    for hook in hooks:
        hook.remove()
    n, L = v * b, h * w
    out = got["out"]
    cot = torch.randn(out.shape, generator=g)
    dq, dk, dv = torch.autograd.grad(out, (got["q"], got["k"], got["v"]), cot)
    flat = lambda t: t.detach().reshape(n, -1, L).contiguous().numpy()  # the reference's .view(b_v, -1, h_down * w_down)
    rec = {"q": flat(got["q"]), "k": flat(got["k"]), "v": flat(got["v"]), "out": flat(out), "cotangent": flat(cot),
           "dq": flat(dq), "dk": flat(dk), "dv": flat(dv)}
    s = torch.einsum("nei,nej->nij", torch.from_numpy(rec["q"]).double(), torch.from_numpy(rec["k"]).double())
    print(f"L = {L}, E = {rec['q'].shape[1]}, C = {rec['v'].shape[1]}, scores {float(s.min()):.1f} .. {float(s.max()):.1f}, "
          f"mean row maximum of p {float(torch.softmax(s, -1).max(-1).values.mean()):.3f}")
    return rec


def main():
    mod = import_reference(sys.argv[1])
    out = {}
    for name, args in RECORDS.items():
        for key, value in run_record(mod, *args).items():
            out[f"{name}.{key}"] = value
    np.savez_compressed(OUT, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
