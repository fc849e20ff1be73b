"""Every header of pf3plat_amd/csrc/ compiles alone: for each csrc/*.h a translation unit of one line, `#include "<header>"`, goes
through hipcc with the product flags (without -shared -fPIC) and -fsyntax-only; gsr_pnp_solver.h, which a host program includes by
itself, through the host C++ compiler as well.  One line per header; exit status 1 if any fails.  No GPU needed.

usage: python tools/check_headers.py"""
import glob
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pf3plat_amd import _lib  # noqa: E402

HOST_TOO = ("gsr_pnp_solver.h",)


def main():
    hip = [_lib.find_hipcc(), *[f for f in _lib.HIPCC_FLAGS if f not in ("-shared", "-fPIC")], "-fsyntax-only"]
    host = [os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++"), "-std=c++17", "-fsyntax-only"]
    failed = 0
    with tempfile.TemporaryDirectory() as tmp:
        for path in sorted(glob.glob(os.path.join(os.path.dirname(_lib.SRC), "*.h"))):
            name = os.path.basename(path)
            for what, cmd, ext in [("hipcc", hip, ".hip")] + ([("host c++", host, ".cpp")] if name in HOST_TOO else []):
                tu = os.path.join(tmp, name[:-2] + ext)
                with open(tu, "w") as f:
                    f.write(f'#include "{path}"\n')
                res = subprocess.run([*cmd, tu], capture_output=True, text=True)
                print(f"{name:20s} {what:9s} {'ok' if res.returncode == 0 else 'FAILED'}")
                if res.returncode != 0:
                    failed += 1
                    print(res.stdout + res.stderr)
    print(f"{failed} failed")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
