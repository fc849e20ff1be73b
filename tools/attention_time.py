"""Measurement aid (GPU box; fails without a device): the pose transformer's multi-head attention
(pf3plat_amd.attention: gsr_attention / gsr_attention_backward) next to eager float32 torch on the SAME device, at PF3plat's sizes
(4 scenes x 3 views of 64 x 64 features plus pose tokens, 4 heads of 32 channels):
  self   (B, H, N, M, D) = (12, 4, 4097, 4097, 32): multi_head_attention against float32 F.scaled_dot_product_attention - what the
         reference's SelfBlock(flash=False) calls.
  cross  (B, H, N, M, D) = (8, 4, 4098, 8196, 32): bidirectional_cross_attention, both m0 and m1, against the reference's einsum lines
         (src/model/LightGlue/lightglue/lightglue.py:210-217) restated below - what its CrossBlock(flash=False) runs.
Legs: the forward (no_grad) and the training step (forward + backward for cotangents on every output, gradients to every input) of
both forms.  After a warm-up the legs alternate in one process; a window is `iters` calls between two device events and ends in a
synchronise; `repeats` windows per leg.  Printed per leg: the median time per call, the spread (min .. max) over the repeats,
torch.cuda.max_memory_allocated over the leg (above what was allocated before it), and the fraction of the f32-input MFMA peak,
157.3 TF, that the algorithm's arithmetic implies at the measured time: 4 B H N M D per attention forward, 2.5 times that again for
its backward (five products: S, dP, dV, dK, dQ; what the kernels recompute on top - S and dP a second time - is not useful work).
One size per process, each under a time limit of its own, the second only if the first ended well:
usage: timeout -k 10 300 python tools/attention_time.py self [iters=20] [repeats=5] && timeout -k 10 600 python tools/attention_time.py cross"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd.attention import bidirectional_cross_attention, multi_head_attention  # noqa: E402

SIZES = {"self": (12, 4, 4097, 4097, 32), "cross": (8, 4, 4098, 8196, 32)}
which = sys.argv[1] if len(sys.argv) > 1 else ""
if which not in SIZES:
    sys.exit(__doc__)
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
if not torch.cuda.is_available():
    sys.exit("tools/attention_time.py measures on the GPU: no device found")
dev = torch.device("cuda:0")
B, H, N, M, D = SIZES[which]
PEAK = 157.3e12  # f32-input MFMA, FLOP per second


def eager_cross(qk0, qk1, v0, v1):
    """lightglue.py:210-217, mask None."""
    scale = D ** -0.5
    qk0, qk1 = qk0 * scale ** 0.5, qk1 * scale ** 0.5
    sim = torch.einsum("bhid, bhjd -> bhij", qk0, qk1)
    attn01 = F.softmax(sim, dim=-1)
    attn10 = F.softmax(sim.transpose(-2, -1).contiguous(), dim=-1)
    m0 = torch.einsum("bhij, bhjd -> bhid", attn01, v1)
    m1 = torch.einsum("bhji, bhjd -> bhid", attn10.transpose(-2, -1), v0)
    return m0, m1


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


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


def main():
    g = torch.Generator().manual_seed(0)
    randn = lambda *s: torch.randn(*s, generator=g).to(dev)
    if which == "self":  # q, k, v as SelfBlock cuts them out of the Wqkv output: interleaved views of one (B, N, 3 H D) buffer
        qkv = (randn(B, N, 3 * H * D) * 2.0).unflatten(-1, (H, -1, 3)).transpose(1, 2)
        inputs = [qkv[..., 0], qkv[..., 1], qkv[..., 2]]
        cots = [randn(B, N, H, D).transpose(1, 2)]
        hip = lambda q, k, v: (multi_head_attention(q, k, v),)
        eager = lambda q, k, v: (F.scaled_dot_product_attention(q.contiguous(), k.contiguous(), v.contiguous()),)  # (lightglue.py:121-122)
        attentions = 1
    else:  # the (B, tokens, H D) projections split into heads, as CrossBlock does
        heads = lambda t: t.unflatten(-1, (H, -1)).transpose(1, 2)
        inputs = [heads(randn(B, N, H * D) * 2.0), heads(randn(B, M, H * D) * 2.0), heads(randn(B, N, H * D)), heads(randn(B, M, H * D))]
        cots = [heads(randn(B, N, H * D)), heads(randn(B, M, H * D))]
        hip = lambda a, b, c, d: bidirectional_cross_attention(a, b, c, d)
        eager = eager_cross
        attentions = 2

    def forward(fn):
        def run():
            with torch.no_grad():
                return fn(*inputs)
        return run

    def step(fn):
        def run():
            leaves = [t.detach().requires_grad_(True) for t in inputs]
            torch.autograd.backward(fn(*leaves), cots)
            return [t.grad for t in leaves]
        return run

    legs = {"HIP   forward": (forward(hip), "forward"), "torch forward": (forward(eager), "forward"),
            "HIP   step": (step(hip), "step"), "torch step": (step(eager), "step")}
    a, t = legs["HIP   forward"][0](), legs["torch forward"][0]()  # the two forms compute the same thing at this size
    ga, gt = legs["HIP   step"][0](), legs["torch step"][0]()
    print("value rel-L2 " + ", ".join(f"{rel_l2(x, y):.2e}" for x, y in zip(a, t)) + "; gradients " + ", ".join(f"{rel_l2(x, y):.2e}" for x, y in zip(ga, gt)))
    del a, t, ga, gt
    for fn, _ in legs.values():  # warm-up: code objects, the allocator, every shape of the timed windows
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(repeats):
        for name, (fn, _) in legs.items():
            times[name].append(window(fn, iters))
    fwd = attentions * 4 * B * H * N * M * D
    flop = {"forward": fwd, "step": 3.5 * fwd}
    med, mem = {}, {}
    print(f"{which}: (B, H, N, M, D) = ({B}, {H}, {N}, {M}, {D}); {repeats} windows of {iters} calls per leg, alternating; microseconds per call")
    for name, (fn, kind) in legs.items():
        ts = sorted(times[name])
        med[name], mem[name] = ts[len(ts) // 2], peak_memory(fn)
        print(f"{name:14s} median {med[name]:10.1f} us   min {ts[0]:10.1f}   max {ts[-1]:10.1f}   peak memory {mem[name] / 2 ** 20:9.1f} MiB   "
              f"{flop[kind] / 1e9:7.1f} GFLOP -> {flop[kind] / (med[name] * 1e-6) / PEAK:6.1%} of 157.3 TF")
    for kind, h, t in (("forward", "HIP   forward", "torch forward"), ("step", "HIP   step", "torch step")):
        spread = max(max(times[h]) - min(times[h]), max(times[t]) - min(times[t]))
        print(f"{kind}: torch / HIP = {med[t] / med[h]:.2f}; difference {med[t] - med[h]:.1f} us against a spread of {spread:.1f} us; "
              f"peak memory torch - HIP = {(mem[t] - mem[h]) / 2 ** 20:.1f} MiB")


if __name__ == "__main__":
    main()
