"""Measurement aid (GPU box; fails without a device): the keypoint extraction (pf3plat_amd.keypoints: gsr_keypoints) next to the
float32 restatement of the reference's lines, run eagerly on the SAME device, at PF3plat's size: 12 images - 4 scenes x 3 views - of 1024 x 1024 pixels
(h = w = 128 cells), C = 256, seeded logits whose dustbin bias leaves a SuperPoint-like 1 - 2 k keypoints per image.
  HIP      one `detect_keypoints` for the twelve images and `Keypoints.lists()`: five launches (six with a top-k cut) and ONE host read.
  torch    the project's float32 restatement of the reference's lines (tests/keypoint_ref.py: `detect`) moved to the device and run
           image by image, each with its `torch.where`, as encoder_costvolume.py:334-337 calls the extractor - twelve host
           synchronisations.
  batched  the same restatement's steps once on the batch of twelve (`batched`, below): one `nonzero` for all images, the split by
           image from its counts, and the descriptor sampling per image on the normalised dense map.  The fairer rival.
  no-desc  (printed last) the batched form without the dense descriptor normalisation and the sampling: what of eager's time is
           the score path.
After a warm-up the legs alternate in one process; a window is `iters` calls between two device events and ends in a synchronise;
`repeats` windows per leg.  Printed per leg: the median time per call, the spread (min .. max) over the repeats, the launches one
call makes (counted with torch.profiler, in a pass of their own after the timing) and torch.cuda.max_memory_allocated over a call
(above what was allocated before it).
usage: timeout -k 10 300 python tools/keypoint_time.py [iters=20] [repeats=5]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd.keypoints import detect_keypoints  # noqa: E402
from tests import keypoint_ref as ref  # noqa: E402

B, HC, WC, C = 12, 128, 128, 256
RADIUS, THRESHOLD, BORDER = 4, 0.0005, 4
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
if not torch.cuda.is_available():
    sys.exit("tools/keypoint_time.py measures on the GPU: no device found")
dev = torch.device("cuda:0")


PARAMS = dict(nms_radius=RADIUS, detection_threshold=THRESHOLD, remove_borders=BORDER, max_num_keypoints=None)


def batched(logits, desc, with_descriptors=True):
    """The restatement's steps on the whole batch at once: per image (keypoints (n, 2) float (x, y), scores (n,), descriptors (n, C))."""
    s = ref.scores_from_logits(logits, torch.float32)
    B, H, W = s.shape
    keep = ref.nms_mask(s, RADIUS) & (s > THRESHOLD)
    keep[:, :BORDER] = False
    keep[:, H - BORDER:] = False
    keep[:, :, :BORDER] = False
    keep[:, :, W - BORDER:] = False
    found = keep.nonzero()  # (image, y, x) in row-major order, image after image: the one host synchronisation
    sizes = torch.bincount(found[:, 0], minlength=B).tolist()
    out = []
    for b, rows in enumerate(found.split(sizes)):
        pix = rows[:, [2, 1]]
        out.append((pix.float(), s[b, rows[:, 1], rows[:, 2]], ref.sample(pix, desc[b], torch.float32) if with_descriptors else None))
    return out


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
    g = torch.Generator().manual_seed(0)
    logits = 2.0 * torch.randn(B, 65, HC, WC, generator=g)
    logits[:, 64] = 14.0 + torch.randn(B, HC, WC, generator=g)  # the dustbin's bias: 1 - 2 k keypoints per image
    logits, desc = logits.to(dev), torch.randn(B, C, HC, WC, generator=g).to(dev)

    def hip():
        return detect_keypoints(logits, desc, nms_radius=RADIUS, detection_threshold=THRESHOLD, remove_borders=BORDER).lists()

    def by_image():
        with torch.no_grad():
            found = [ref.detect(logits[b:b + 1], desc[b:b + 1], None, PARAMS, torch.float32)[0] for b in range(B)]
        return [(f["keypoints"], f["keypoint_scores"], f["descriptors"]) for f in found]

    def whole_batch():
        with torch.no_grad():
            return batched(logits, desc)

    def no_descriptors():
        with torch.no_grad():
            return batched(logits, desc, with_descriptors=False)

    mine, theirs = hip(), by_image()
    counts = [t[0].shape[0] for t in theirs]
    same = sum(int(torch.equal(a["keypoints"], b[0])) for a, b in zip(mine, theirs))
    worst = max([float((a["descriptors"].double() - b[2].double()).norm() / b[2].double().norm()) for a, b in zip(mine, theirs)
                 if torch.equal(a["keypoints"], b[0]) and b[0].shape[0]] or [float("nan")])
    print(f"keypoints per image: {counts}; {same} of {B} images with identical keypoints; descriptors rel-L2 at most {worst:.2e} on those")
    legs = {"HIP    ": hip, "torch  ": by_image, "batched": whole_batch, "no-desc": no_descriptors}
    for fn in legs.values():  # warm-up: code objects, the allocator, every shape of the timed windows
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(repeats):
        for name, fn in legs.items():
            times[name].append(window(fn, iters))
    print(f"{B} images of {8 * HC} x {8 * WC}, C = {C}; {repeats} windows of {iters} calls per leg, alternating; microseconds per call (lists included)")
    med, mem = {}, {}
    for name, fn in legs.items():
        ts = sorted(times[name])
        med[name], mem[name] = ts[len(ts) // 2], peak_memory(fn)
        print(f"{name} median {med[name]:10.1f} us   min {ts[0]:10.1f}   max {ts[-1]:10.1f}   launches {launches(fn)}   peak memory {mem[name] / 2 ** 20:8.2f} MiB")
    spread = max(max(t) - min(t) for t in times.values())
    print(f"torch / HIP = {med['torch  '] / med['HIP    ']:.2f}, batched / HIP = {med['batched'] / med['HIP    ']:.2f} (spread of a leg at most {spread:.1f} us); "
          f"of batched's {med['batched']:.1f} us the descriptor path is {med['batched'] - med['no-desc']:.1f} us")


if __name__ == "__main__":
    main()
