"""Measurement aid (GPU box; fails without a device): LightGlue's transformer on the device (pf3plat_amd.matcher; the attention is
gsr_ragged_attention) next to the reference's eager float32 lines on the SAME device, at PF3plat's size: 12 lists - 4 scenes x 3 pairs -
of 1024 x 1024 keypoints, d = 256, 4 heads of 64, 9 layers.
  HIP self / cross   one `ragged_attention` launch for the 24 units: the self-attention with the rotary encoding, q, k and v read out of
                     the interleaved Wqkv output; both directions of the cross-attention.
  torch self / cross the reference's lines (src/model/LightGlue/lightglue/lightglue.py:57-58, 120-123, 158-164, 210-217, restated
                     below) list by list: its torch rotary and F.scaled_dot_product_attention on contiguous copies; its einsum branch.
  HIP / torch matcher the whole LightGlue.forward - encoding, 9 layers, assignment, the lists - against the reference's list by list
                     with the same weights.
After a warm-up the legs alternate in one process; a window is `iters` calls between two device events and ends in a synchronise;
`repeats` windows per leg.  Printed per leg: the median time per call, the spread (min .. max) over the repeats,
torch.cuda.max_memory_allocated over a call (above what was allocated before it) and, for the attention legs, the fraction of the
157.3 TFLOP/s f32 MFMA peak that 4 H D sum n_u m_u FLOP per launch imply.
usage: timeout -k 10 600 python tools/matcher_time.py [iters=20] [repeats=5]"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd.attention import apply_cached_rotary_emb, ragged_attention  # noqa: E402
from pf3plat_amd.matcher import LightGlue, list_layout, normalize_keypoints  # noqa: E402
from pf3plat_amd.matching import match_assignment  # noqa: E402

L, M, N, DIM, H, LAYERS, SIZE = 12, 1024, 1024, 256, 4, 9, (640, 480)
D = DIM // H
PEAK = 157.3e12
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
if not torch.cuda.is_available():
    sys.exit("tools/matcher_time.py measures on the GPU: no device found")
dev = torch.device("cuda:0")


def eager_self(qkv, enc):
    """SelfBlock.forward up to the context for one list: qkv (1, n, 3 DIM) the Wqkv output, enc (2, 1, 1, n, D)."""
    qkv = qkv.unflatten(-1, (H, -1, 3)).transpose(1, 2)
    q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
    q, k = apply_cached_rotary_emb(enc, q), apply_cached_rotary_emb(enc, k)
    return F.scaled_dot_product_attention(q.contiguous(), k.contiguous(), v.contiguous())


def eager_cross(qk0, qk1, v0, v1):
    """CrossBlock.forward's einsum branch for one list: (1, H, n, D) operands."""
    scale = D ** -0.5
    qk0, qk1 = qk0 * scale ** 0.5, qk1 * scale ** 0.5
    sim = torch.einsum("bhid, bhjd -> bhij", qk0, qk1)
    attn01 = F.softmax(sim, dim=-1)
    attn10 = F.softmax(sim.transpose(-2, -1).contiguous(), dim=-1)
    return torch.einsum("bhij, bhjd -> bhid", attn01, v1), torch.einsum("bhji, bhjd -> bhid", attn10.transpose(-2, -1), v0)


def eager_matcher(model, desc0, desc1, kpts0, kpts1):
    """LightGlue._forward without pruning or early stop for one list (batch 1), on the module's weights."""
    enc0, enc1 = (model.posenc(normalize_keypoints(k, SIZE)) for k in (kpts0, kpts1))
    x0, x1 = model.input_proj(desc0), model.input_proj(desc1)
    heads = lambda t: t.unflatten(-1, (H, -1)).transpose(1, 2)
    for layer in model.transformers:
        s, c = layer.self_attn, layer.cross_attn
        for side in (0, 1):
            x, enc = (x0, enc0) if side == 0 else (x1, enc1)
            context = eager_self(s.Wqkv(x), enc)
            x = x + s.ffn(torch.cat([x, s.out_proj(context.transpose(1, 2).flatten(start_dim=-2))], -1))
            x0, x1 = (x, x1) if side == 0 else (x0, x)
        m0, m1 = eager_cross(heads(c.to_qk(x0)), heads(c.to_qk(x1)), heads(c.to_v(x0)), heads(c.to_v(x1)))
        m0, m1 = (c.to_out(m.transpose(1, 2).flatten(start_dim=-2)) for m in (m0, m1))
        x0, x1 = x0 + c.ffn(torch.cat([x0, m0], -1)), x1 + c.ffn(torch.cat([x1, m1], -1))
    head = model.log_assignment[-1]
    return match_assignment(head.final_proj(x0), head.final_proj(x1), head.matchability(x0), head.matchability(x1)).lists()


def window(fn, count):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(count):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return 1e3 * start.elapsed_time(stop) / count  # microseconds per call


def peak_memory(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


@torch.no_grad()
def main():
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    model = LightGlue(n_layers=LAYERS).to(dev).eval()
    desc0, desc1 = torch.randn(L * M, DIM, generator=g), torch.randn(L * N, DIM, generator=g)
    wh = torch.tensor(SIZE, dtype=torch.float32)
    kpts0, kpts1 = torch.rand(L * M, 2, generator=g) * (wh - 1), torch.rand(L * N, 2, generator=g) * (wh - 1)
    desc0, desc1, kpts0, kpts1 = (t.to(dev) for t in (desc0, desc1, kpts0, kpts1))
    len0, len1 = (M,) * L, (N,) * L
    lay = list_layout(len0, len1)
    T = L * (M + N)
    x = torch.cat([desc0, desc1])
    rot = model.posenc(normalize_keypoints(torch.cat([kpts0, kpts1]), SIZE))[:, 0].contiguous()
    first = model.transformers[0]
    qkv = first.self_attn.Wqkv(x)
    q4 = qkv.view(T, H, D, 3)
    qk, v = first.cross_attn.to_qk(x).view(T, H, D), first.cross_attn.to_v(x).view(T, H, D)
    units = [(b, c) for b, c in lay.self_ranges]
    encs = [rot[:, b:b + c][:, None, None] for b, c in units]  # (2, 1, 1, n, D) per unit
    lists = [((o, M), (L * M + p, N)) for o, p in zip(lay.offsets0[:-1], lay.offsets1[:-1])]
    heads = lambda t: t[None].transpose(1, 2)  # (n, H, D) -> (1, H, n, D)

    legs = {
        "HIP self    ": lambda: ragged_attention(q4[..., 0], q4[..., 1], q4[..., 2], lay.self_ranges, lay.self_ranges, rot=rot),
        "torch self  ": lambda: [eager_self(qkv[None, b:b + c], e) for (b, c), e in zip(units, encs)],
        "HIP cross   ": lambda: ragged_attention(qk, qk, v, lay.cross_q, lay.cross_k, scale=D ** -0.5),
        "torch cross ": lambda: [eager_cross(heads(qk[a:a + m]), heads(qk[b:b + n]), heads(v[a:a + m]), heads(v[b:b + n])) for (a, m), (b, n) in lists],
        "HIP matcher ": lambda: model(desc0, desc1, kpts0, kpts1, len0, len1, SIZE).lists(),
        "torch matcher": lambda: [eager_matcher(model, desc0[None, a:a + m], desc1[None, b - L * M:b - L * M + n], kpts0[None, a:a + m],
                                                kpts1[None, b - L * M:b - L * M + n]) for (a, m), (b, n) in lists],
    }
    # what the two paths compute is the same: the self context and the final matches
    mine = legs["HIP self    "]()
    theirs = torch.cat([o[0].transpose(0, 1) for o in legs["torch self  "]()])
    print(f"self context, HIP against torch: rel-L2 {float((mine - theirs).norm() / theirs.norm()):.2e}")
    a, b = legs["HIP matcher "](), legs["torch matcher"]()
    same = sum(int(torch.equal(p[0], q[0][0])) for p, q in zip(a, b))
    print(f"{same} of {L} lists with identical matches ({sum(len(p[0]) for p in a)} matches in all)")
    flop = {"self": 4.0 * H * D * sum(c * c for _, c in units), "cross": 4.0 * H * D * 2 * L * M * N}
    for fn in legs.values():  # warm-up: code objects, the allocator, every shape of the timed windows
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            times[name].append(window(fn, iters if "matcher" not in name else max(iters // 4, 1)))
    print(f"{L} lists of {M} x {N}, d = {DIM}, {H} heads, {LAYERS} layers; {repeats} windows of {iters} calls per leg ({max(iters // 4, 1)} for the whole "
          "matcher), alternating; microseconds per call")
    med = {}
    for name, fn in legs.items():
        ts = sorted(times[name])
        med[name] = ts[len(ts) // 2]
        kind = name.split()[1]
        frac = f"   {100 * flop[kind] / (med[name] * 1e-6) / PEAK:5.1f} % of the f32 MFMA peak" if kind in flop else ""
        print(f"{name} median {med[name]:10.1f} us   min {ts[0]:10.1f}   max {ts[-1]:10.1f}   peak memory {peak_memory(fn) / 2 ** 20:8.2f} MiB{frac}")
    for kind in ("self", "cross", "matcher"):
        t, h = (next(v for k, v in med.items() if k.startswith(path) and kind in k) for path in ("torch", "HIP"))
        print(f"{kind}: torch / HIP = {t / h:.2f}")


if __name__ == "__main__":
    main()
