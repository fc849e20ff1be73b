"""Compare the device code of two builds kernel by kernel: the gate for a change that must not move device code.  No GPU needed.
Prints the kernels only one side has, the kernels whose instruction bytes, kernel descriptor or metadata note (VGPR / AGPR /
SGPR counts, LDS, private segment, kernarg size, ...) differ, and the symbols whose address or size moved - counted are the FUNC and OBJECT symbols by name, which here are the kernels and
their .kd descriptors (two per kernel; not __hip_cuid_*, whose name is a hash of the source): a kernel that only sits at another address
computes the same, but not at the same speed - the layout of a hot loop in the instruction cache moves with it (two instances that
swapped places cost the single-view forward 0.2 us: docs/KERNEL_HISTORY.md).  Exit status 1 if anything differs or moved.
--ignore-addresses: for a change that adds or removes kernels on purpose, compare the common ones without their addresses.

usage: python tools/compare_code_objects.py [--ignore-addresses] OLD.co NEW.co
       python tools/compare_code_objects.py --build OUT.co [extra hipcc flags...]   (this tree's csrc/gsr_hip.hip -> OUT.co)
For the other side, --build in a checkout of the other commit (git worktree add DIR COMMIT)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd import _lib  # noqa: E402

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def llvm(tool):
    return os.path.join(os.path.dirname(os.path.realpath(_lib.find_hipcc())), "..", "lib", "llvm", "bin", tool)


def build(out, extra_flags):
    flags = [f for f in _lib.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([_lib.find_hipcc(), *flags, *extra_flags, "--cuda-device-only", "-c", "-o", out + ".bundle", _lib.SRC], check=True)
    subprocess.run([llvm("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={out}.bundle", f"--output={out}"], check=True)
    os.remove(out + ".bundle")


def kernels(path):
    """{kernel name: (instruction bytes, descriptor bytes without the entry offset, {note key: value})}, {symbol: (address, size)}"""
    out = subprocess.run([llvm("llvm-readelf"), "-SW", "-sW", "--notes", path], capture_output=True, text=True, check=True).stdout
    data = open(path, "rb").read()
    sections = {int(m[1]): (int(m[2], 16), int(m[3], 16)) for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s", out, re.M)}
    symbols, places = {}, {}
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]{16})\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", out, re.M):
        addr, off = sections[int(m[4])]
        start = off + int(m[1], 16) - addr
        symbols[m[5]] = data[start:start + int(m[2])]
        if not m[5].startswith("__hip_cuid_"):
            places[m[5]] = (int(m[1], 16), int(m[2]))
    notes = {}
    for entry in re.split(r"^  - (?=\.)", out[out.index("amdhsa.kernels:"):], flags=re.M)[1:]:
        entry = "    " + entry.split("\namdhsa.")[0]
        fields = dict(re.findall(r"^    (\.\w+):\s+(\S.*)$", entry, re.M))
        fields[".args"] = re.sub(r"\s+", " ", entry[entry.index(".args:"):entry.index("    .group_segment_fixed_size")]) if ".args:" in entry else ""
        notes[fields.pop(".name")] = fields
    # (bytes 16..23 of a descriptor: the offset from it to the kernel's entry, which moves with the kernel)
    return {n: (symbols[n], symbols[n + ".kd"][:16] + symbols[n + ".kd"][24:], notes[n]) for n in notes}, places


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "--build":
        return build(sys.argv[2], sys.argv[3:])
    args = [a for a in sys.argv[1:] if a != "--ignore-addresses"]
    addresses = len(args) == len(sys.argv) - 1
    if len(args) != 2:
        sys.exit(__doc__)
    (old, old_at), (new, new_at) = kernels(args[0]), kernels(args[1])
    differ = 0
    for n in sorted(set(old) ^ set(new)):
        differ += 1
        print(f"only in {'OLD' if n in old else 'NEW'}: {n}")
    for n in sorted(set(old) & set(new)):
        (code_a, kd_a, note_a), (code_b, kd_b, note_b) = old[n], new[n]
        what = []
        if code_a != code_b:
            first = next((i for i, (x, y) in enumerate(zip(code_a, code_b)) if x != y), min(len(code_a), len(code_b)))
            what.append(f"instructions ({len(code_a)} -> {len(code_b)} bytes, first difference at byte {first})")
        if kd_a != kd_b:
            what.append("kernel descriptor")
        what += [f"{k}: {note_a.get(k)} -> {note_b.get(k)}" for k in sorted(set(note_a) | set(note_b)) if note_a.get(k) != note_b.get(k)]
        if what:
            differ += 1
            print(f"differs: {n}: " + "; ".join(what))
    if addresses:
        moved = 0
        for n in sorted(set(old_at) | set(new_at), key=lambda n: (old_at.get(n) or new_at[n], n)):
            if old_at.get(n) != new_at.get(n):
                moved += 1
                at = lambda place: "absent" if place is None else f"{place[0]:#x} + {place[1]}"
                print(f"moved: {n}: {at(old_at.get(n))} -> {at(new_at.get(n))}")
        print(f"{len(old)} kernels in OLD, {len(new)} in NEW, {differ} differ, {moved} of {len(set(old_at) | set(new_at))} symbols moved")
        sys.exit(1 if differ or moved else 0)
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW, {differ} differ (addresses not compared)")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
