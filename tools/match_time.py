"""Measurement aid (GPU box; fails without a device): the matcher's assignment (pf3plat_amd.matching: gsr_match_assignment) next to the
reference's eager float32 lines on the SAME device, at PF3plat's size: 12 lists - 4 scenes x 3 pairs - of 1024 x 1024 keypoints,
d = 256 (roughly the match counts the README's coarse-pose row assumes).
  HIP    one `match_assignment` for the twelve lists and `Matches.lists()`: three launches and ONE host read.
  torch  the reference's lines (src/model/LightGlue/lightglue/lightglue.py:283-289, 259-271, 296-312, 588-597, restated below) run
         list by list, each with its `torch.where` - twelve host synchronisations.
After a warm-up the two legs alternate in one process; a window is `iters` calls between two device events and ends in a
synchronise; `repeats` windows per leg.  Printed per leg: the median time per call, the spread (min .. max) over the repeats and
torch.cuda.max_memory_allocated over a call (above what was allocated before it).
usage: timeout -k 10 300 python tools/match_time.py [iters=20] [repeats=5]"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd.matching import match_assignment  # noqa: E402

L, M, N, D = 12, 1024, 1024, 256
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
if not torch.cuda.is_available():
    sys.exit("tools/match_time.py measures on the GPU: no device found")
dev = torch.device("cuda:0")


def eager_list(mdesc0, mdesc1, z0, z1, th=0.1):
    """One list, batch 1: MatchAssignment.forward after its projections, sigmoid_log_double_softmax, filter_matches, the list."""
    _, m, d = mdesc0.shape
    n = mdesc1.shape[1]
    mdesc0, mdesc1 = mdesc0 / d ** 0.25, mdesc1 / d ** 0.25
    sim = torch.einsum("bmd,bnd->bmn", mdesc0, mdesc1)
    certainties = F.logsigmoid(z0) + F.logsigmoid(z1).transpose(1, 2)
    scores0 = F.log_softmax(sim, 2)
    scores1 = F.log_softmax(sim.transpose(-1, -2).contiguous(), 2).transpose(-1, -2)
    scores = sim.new_full((1, m + 1, n + 1), 0)
    scores[:, :m, :n] = scores0 + scores1 + certainties
    scores[:, :-1, -1] = F.logsigmoid(-z0.squeeze(-1))
    scores[:, -1, :-1] = F.logsigmoid(-z1.squeeze(-1))
    max0, max1 = scores[:, :-1, :-1].max(2), scores[:, :-1, :-1].max(1)
    m0, m1 = max0.indices, max1.indices
    indices0 = torch.arange(m0.shape[1], device=m0.device)[None]
    indices1 = torch.arange(m1.shape[1], device=m1.device)[None]
    mutual0 = indices0 == m1.gather(1, m0)
    mutual1 = indices1 == m0.gather(1, m1)
    max0_exp = max0.values.exp()
    zero = max0_exp.new_tensor(0)
    mscores0 = torch.where(mutual0, max0_exp, zero)
    mscores1 = torch.where(mutual1, mscores0.gather(1, m1), zero)
    valid0 = mutual0 & (mscores0 > th)
    valid1 = mutual1 & valid0.gather(1, m1)
    m0 = torch.where(valid0, m0, -1)
    m1 = torch.where(valid1, m1, -1)
    valid = m0[0] > -1
    return torch.stack([torch.where(valid)[0], m0[0][valid]], -1), mscores0[0][valid], m1, mscores1


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
    x0 = torch.randn(L, M, D, generator=g)
    x1 = torch.randn(L, N, D, generator=g)
    half = M // 2  # half of each list's keypoints have a partner
    for l in range(L):
        i, j = torch.randperm(M, generator=g)[:half], torch.randperm(N, generator=g)[:half]
        x1[l, j] = x0[l, i] + 0.1 * torch.randn(half, D, generator=g)
    w = torch.randn(D, D, generator=g) * (2.0 / D ** 0.5)
    a0, a1 = (x0 @ w.T).to(dev), (x1 @ w.T).to(dev)
    z0, z1 = (2.0 * torch.randn(L, M, 1, generator=g) + 1.0).to(dev), (2.0 * torch.randn(L, N, 1, generator=g) + 1.0).to(dev)

    def hip():
        return match_assignment(a0, a1, z0, z1).lists()

    def eager():
        with torch.no_grad():
            return [eager_list(a0[l:l + 1], a1[l:l + 1], z0[l:l + 1], z1[l:l + 1])[:2] for l in range(L)]

    mine, theirs = hip(), eager()
    same = sum(int(torch.equal(a[0], b[0])) for a, b in zip(mine, theirs))
    found = sum(a[0].shape[0] for a in theirs)
    worst = max(float((a[1].double() - b[1].double()).norm() / b[1].double().norm()) for a, b in zip(mine, theirs) if torch.equal(a[0], b[0]) and a[0].shape[0]) if same else float('nan')
    print(f"{same} of {L} lists with identical matches ({found} matches in all); scores rel-L2 at most {worst:.2e} on those")
    legs = {"HIP  ": hip, "torch": eager}
    for fn in legs.values():  # warm-up: code objects, the allocator, every shape of the timed windows
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            times[name].append(window(fn, iters))
    print(f"{L} lists of {M} x {N}, d = {D}; {repeats} windows of {iters} calls per leg, alternating; microseconds per call (lists included)")
    med, mem = {}, {}
    for name, fn in legs.items():
        ts = sorted(times[name])
        med[name], mem[name] = ts[len(ts) // 2], peak_memory(fn)
        print(f"{name} median {med[name]:10.1f} us   min {ts[0]:10.1f}   max {ts[-1]:10.1f}   peak memory {mem[name] / 2 ** 20:8.2f} MiB")
    spread = max(max(t) - min(t) for t in times.values())
    print(f"torch / HIP = {med['torch'] / med['HIP  ']:.2f}; difference {med['torch'] - med['HIP  ']:.1f} us against a spread of {spread:.1f} us; "
          f"peak memory torch - HIP = {(mem['torch'] - mem['HIP  ']) / 2 ** 20:.2f} MiB")


if __name__ == "__main__":
    main()
