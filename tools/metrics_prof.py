"""Measurement aid (GPU box), sibling of tools/loss_prof.py: the evaluation-metrics launch pair (gsr_image_metrics +
gsr_image_metrics_finish) next to the image-loss pair without a gradient pointer (gsr_image_loss + gsr_image_loss_finish) on
V x 3 x 256 x 256 images, in ONE process and alternating blocks, so that both see the same machine.  Two figures each: wall per call
through pf3plat_amd.losses (allocations and Python included) and wall per launch pair through the C ABI on preallocated buffers
(host clock around `reps` enqueued pairs that end in a synchronise).  Under rocprofv3 --kernel-trace --stats: the kernels' own times.
usage: python tools/metrics_prof.py [reps=2000] [rounds=5] [V ...=3 12]"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd import _lib, losses  # noqa: E402
from pf3plat_amd.rasterizer import _stream_ptr  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
views = [int(a) for a in sys.argv[3:]] or [3, 12]
dev = torch.device("cuda:0")
lib = _lib.load()


def timed(fn, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / count


for V in views:
    g = torch.Generator().manual_seed(0)
    pred = torch.rand((V, 3, 256, 256), generator=g).to(dev)
    tgt = torch.rand((V, 3, 256, 256), generator=g).to(dev)
    slots = int(lib.gsr_image_metrics_partials(V, 256, 256))
    partials = torch.empty((slots, 4), device=dev)
    out = torch.empty((V + 1, 4), device=dev)
    smap = torch.empty_like(pred)
    stream = _stream_ptr(dev)
    p, t, pp, o, o_tot, sm = pred.data_ptr(), tgt.data_ptr(), partials.data_ptr(), out.data_ptr(), out[V].data_ptr(), smap.data_ptr()

    def c_loss():
        lib.gsr_image_loss(V, 256, 256, p, t, 1.0, 0.05, None, pp, stream)
        lib.gsr_image_loss_finish(V, 256, 256, pp, 1.0, 0.05, o, o_tot, stream)

    def c_metrics():
        lib.gsr_image_metrics(V, 256, 256, t, p, None, pp, stream)
        lib.gsr_image_metrics_finish(V, 256, 256, pp, o, stream)

    def c_metrics_map():
        lib.gsr_image_metrics(V, 256, 256, t, p, sm, pp, stream)
        lib.gsr_image_metrics_finish(V, 256, 256, pp, o, stream)

    legs = {"C ABI  image_loss pair, no gradient": c_loss, "C ABI  image_metrics pair": c_metrics, "C ABI  image_metrics pair + map": c_metrics_map,
            "Python losses._launch, no gradient": lambda: losses._launch(pred, tgt, 1.0, 0.05, False),
            "Python compute_image_metrics": lambda: losses.compute_image_metrics(tgt, pred)}
    for fn in legs.values():
        timed(fn, 50)
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(timed(fn, reps))
    for name, ts in times.items():
        print(f"V={V:2d} {name:38s} median {sorted(ts)[len(ts) // 2]:7.2f} us   min {min(ts):7.2f}   max {max(ts):7.2f}   ({rounds} x {reps} calls)")
