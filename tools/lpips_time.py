"""Measurement aid (GPU box; fails without a device): the perceptual distance's head (pf3plat_amd.lpips: gsr_lpips_head, _finish,
_backward) next to the package's lines restated in eager float32 torch (tests/lpips_ref.py: `upstream_head`, `pipeline`) on the SAME
device, at PF3plat's training size: 12 pairs - the inner target views of a batch - of 256 x 256 pixels, i.e. five feature pyramids
of 64 x 256^2 + 128 x 128^2 + 256 x 64^2 + 512 x 32^2 + 512 x 16^2 = 7 995 392 floats per image and side.
  head fwd     the head alone on seeded relu(3 N(0, 1)) features, no gradient: two launches against the eager lines.
  head step    forward and backward with the gradient going to side a (the prediction), as in training: three launches.
  module step  the whole `LPIPS` module, normalize=True, forward and backward to in0: the same 13 torch convolutions on either
               side (seeded random weights), so the difference of the two legs is the head's.
After a warm-up the legs alternate in one process; a window is `iters` calls between two device events and ends in a synchronise;
`repeats` windows per leg.  Printed per leg: the median time per call, the spread (min .. max) over the repeats, the launches one
call makes (counted with torch.profiler, in a pass of their own after the timing), torch.cuda.max_memory_allocated over a call
above what was allocated before it (the operands), and for the head the fraction of the 8 TB/s roofline its algorithmic bytes
imply: forward 2 x 12 x 7 995 392 x 4 = 768 MB read; step that twice plus 384 MB written.
usage: timeout -k 10 600 python tools/lpips_time.py [iters=20] [repeats=5]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd.lpips import LPIPS, VGG_CHANNELS, lpips_distance  # noqa: E402
from tests import lpips_ref as ref  # noqa: E402

N, SIDE = 12, 256
ROOFLINE = 8e12
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
if not torch.cuda.is_available():
    sys.exit("tools/lpips_time.py measures on the GPU: no device found")
dev = torch.device("cuda:0")


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


def main():
    g = torch.Generator(device=dev).manual_seed(0)
    shapes = [(N, c, SIDE >> l, SIDE >> l) for l, c in enumerate(VGG_CHANNELS)]
    fa = [torch.relu(3 * torch.randn(s, generator=g, device=dev)) for s in shapes]
    fb = [torch.relu(3 * torch.randn(s, generator=g, device=dev)) for s in shapes]
    ws = [torch.rand(c, generator=g, device=dev) for c in VGG_CHANNELS]
    floats = sum(t.numel() for t in fa)
    fwd_bytes, step_bytes = 2 * floats * 4, (2 * 2 + 1) * floats * 4
    module = LPIPS(seed=0).to(dev)
    buffers = dict(module.named_buffers())
    in0, in1 = torch.rand((N, 3, SIDE, SIDE), generator=g, device=dev), torch.rand((N, 3, SIDE, SIDE), generator=g, device=dev)
    leaves = [t.clone().requires_grad_() for t in fa]
    image = in0.clone().requires_grad_()

    def hip_fwd():
        with torch.no_grad():
            return lpips_distance(fa, fb, ws)[0]

    def eager_fwd():
        with torch.no_grad():
            return ref.upstream_head(fa, fb, ws)[:, 0, 0, 0]

    def step(head):
        for t in leaves:
            t.grad = None
        head(leaves).sum().backward()
        return leaves[0].grad

    def hip_step():
        return step(lambda xs: lpips_distance(xs, fb, ws)[0])

    def eager_step():
        return step(lambda xs: ref.upstream_head(xs, fb, ws))

    def hip_module():
        image.grad = None
        module(image, in1, normalize=True).sum().backward()
        return image.grad

    def eager_module():
        image.grad = None
        ref.pipeline(buffers, image, in1, torch.float32, normalize=True).sum().backward()
        return image.grad

    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())  # noqa: E731
    print(f"the two forms agree: values rel-L2 {rel(hip_fwd(), eager_fwd()):.2e}, dL/da of layer 0 {rel(hip_step().clone(), eager_step().clone()):.2e}, "
          f"module dL/din0 {rel(hip_module().clone(), eager_module().clone()):.2e}")
    legs = {"head fwd    HIP  ": hip_fwd, "head fwd    eager": eager_fwd, "head step   HIP  ": hip_step, "head step   eager": eager_step,
            "module step HIP  ": hip_module, "module step eager": eager_module}
    for fn in legs.values():  # warm-up: code objects, the convolutions' algorithm search, the allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            times[name].append(window(fn, iters))
    print(f"{N} pairs of {SIDE} x {SIDE}: {floats / N:.0f} feature floats per image and side; {repeats} windows of {iters} calls per leg, alternating; microseconds per call")
    med = {}
    for name, fn in legs.items():
        ts = sorted(times[name])
        med[name] = ts[len(ts) // 2]
        roof = ""
        if name.startswith("head"):
            nbytes = fwd_bytes if "fwd" in name else step_bytes
            roof = f"   {nbytes / 1e6:.0f} MB: {nbytes / ROOFLINE / (med[name] * 1e-6):.3f} of the 8 TB/s roofline"
        print(f"{name} median {med[name]:10.1f} us   min {ts[0]:10.1f}   max {ts[-1]:10.1f}   launches {launches(fn)}   "
              f"peak memory {peak_memory(fn) / 2 ** 20:9.1f} MiB{roof}")
    for kind in ("head fwd   ", "head step  ", "module step"):
        print(f"{kind}: eager / HIP = {med[kind + ' eager'] / med[kind + ' HIP  ']:.2f}")
    print(f"module step: eager - HIP = {med['module step eager'] - med['module step HIP  ']:.1f} us; head step: eager - HIP = "
          f"{med['head step   eager'] - med['head step   HIP  ']:.1f} us")


if __name__ == "__main__":
    main()
