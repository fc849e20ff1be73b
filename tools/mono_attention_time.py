"""Measurement aid (GPU box; fails without a device): the depth predictor's mono-guided attention
(pf3plat_amd.mono_attention.mono_guided_attention: gsr_mono_attention / gsr_mono_attention_backward) next to the reference's five eager
lines in float32 on the SAME device - tests/mono_attention_ref.attention, which is not the code under test.  At PF3plat's size:
(n, E, L, C) = (8, 8, 4096, 128), 4 scenes x 2 context views of 64 x 64 features.  Legs: the forward (no_grad) and the training step
(forward + backward for a cotangent on the output, gradients to q, k and v) of both forms.  After a warm-up the legs alternate in one
process; a window is `iters` calls between two device events and ends in a synchronise; `repeats` windows per leg.  Printed per leg:
the median time per call, the spread (min .. max) over the repeats, the launches one call makes (counted with torch.profiler, in a
pass of their own after the timing), torch.cuda.max_memory_allocated over the leg (above what was allocated before it), and the
fraction of the f32-input MFMA peak, 157.3 TF, that the algorithm's arithmetic implies at the measured time: 2 n L^2 (E + C) for the
forward, about 3.1 times that for the step (the backward's five products: S, dP, dV over C and dK, dQ over E count 2 n L^2 (2 C + 3 E); what
the kernels recompute on top - S and dP a second time - is not counted as useful work).
usage: python tools/mono_attention_time.py [iters=20] [repeats=5]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd.mono_attention import mono_guided_attention  # noqa: E402
from tests import mono_attention_ref as ref  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
if not torch.cuda.is_available():
    sys.exit("tools/mono_attention_time.py measures on the GPU: no device found")
dev = torch.device("cuda:0")
N, E, L, C = 8, 8, 4096, 128
PEAK = 157.3e12  # f32-input MFMA, FLOP per second


def useful_flop():
    fwd = 2 * N * L * L * (E + C)
    bwd = 2 * N * L * L * (2 * C + 3 * E)
    return {"forward": fwd, "step": fwd + bwd}


def window(fn, count):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(count):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return 1e3 * start.elapsed_time(stop) / count  # microseconds per call


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as e:  # noqa: BLE001
        return f"not counted ({type(e).__name__})"


def peak_memory(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    case = ref.build_case(0, N, E, L, C, 4.0, "random")
    q, k, v, cot = (case[key].to(dev) for key in ("q", "k", "v", "cotangent"))
    eager = lambda a, b, c: ref.attention(a, b, c, torch.float32)

    def forward(fn):
        def run():
            with torch.no_grad():
                return fn(q.permute(0, 2, 1), k, v)
        return run

    def step(fn):
        def run():
            qg, kg, vg = (t.detach().requires_grad_(True) for t in (q, k, v))
            fn(qg.permute(0, 2, 1), kg, vg).backward(cot)
            return qg.grad, kg.grad, vg.grad
        return run

    legs = {"HIP   forward": (forward(mono_guided_attention), "forward"), "torch forward": (forward(eager), "forward"),
            "HIP   step": (step(mono_guided_attention), "step"), "torch step": (step(eager), "step")}
    # the two forms compute the same thing at this size
    a, t = legs["HIP   forward"][0](), legs["torch forward"][0]()
    ga, gt = legs["HIP   step"][0](), legs["torch step"][0]()
    print(f"value rel-L2 {ref.rel_l2(a, t):.2e}; gradients dq {ref.rel_l2(ga[0], gt[0]):.2e}, dk {ref.rel_l2(ga[1], gt[1]):.2e}, dv {ref.rel_l2(ga[2], gt[2]):.2e}")
    del a, t, ga, gt
    for fn, _ in legs.values():  # warm-up: code objects, the allocator, every shape of the timed windows
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(repeats):
        for name, (fn, _) in legs.items():
            times[name].append(window(fn, iters))
    flop = useful_flop()
    med, mem = {}, {}
    print(f"(n, E, L, C) = ({N}, {E}, {L}, {C}); {repeats} windows of {iters} calls per leg, alternating; microseconds per call")
    for name, (fn, kind) in legs.items():
        ts = sorted(times[name])
        med[name], mem[name] = ts[len(ts) // 2], peak_memory(fn)
        print(f"{name:14s} median {med[name]:10.1f} us   min {ts[0]:10.1f}   max {ts[-1]:10.1f}   launches {launches(fn)}   "
              f"peak memory {mem[name] / 2 ** 20:8.1f} MiB   {flop[kind] / 1e9:6.1f} GFLOP -> {flop[kind] / (med[name] * 1e-6) / PEAK:6.1%} of 157.3 TF")
    for kind, h, t in (("forward", "HIP   forward", "torch forward"), ("step", "HIP   step", "torch step")):
        spread = max(max(times[h]) - min(times[h]), max(times[t]) - min(times[t]))
        print(f"{kind}: torch / HIP = {med[t] / med[h]:.2f}; difference {med[t] - med[h]:.1f} us against a spread of {spread:.1f} us; "
              f"peak memory torch - HIP = {(mem[t] - mem[h]) / 2 ** 20:.1f} MiB")


if __name__ == "__main__":
    main()
