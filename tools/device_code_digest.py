#!/usr/bin/env python3
"""One digest per kernel translation unit of what the gfx950 code object holds.

For every object of the Makefile's OBJS except host.o: compile the device side alone with the flags the
Makefile gives that unit (taken from `make -n`, so a per-unit EXTRA is included) plus --cuda-device-only,
unbundle the gfx950 code object, and hash `llvm-objdump -d` together with `llvm-readelf --notes`, without the
lines that print the file's own name. Two checkouts whose lists are equal run the same device code: a
refactor of the launch layer compares its list with the parent's (profiles/launch_layer_device_code.txt).
The compiler is not perfectly repeatable under load (the same source gave a second code object in about one
compile in twenty of some units): compile a unit that differs again, by name, before it counts as a difference.

    python tools/device_code_digest.py [--csrc DIR] [--jobs N] [unit ...]     # prints "unit digest" lines
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def units_of(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    objs = re.search(r"^OBJS := (.*)$", text, re.M).group(1).split()
    return [o[:-2] for o in objs if o != "host.o"]


def compile_line(csrc, unit):
    out = subprocess.run(["make", "-C", csrc, "-n", "-B", "--no-print-directory", unit + ".o"], check=True,
                         capture_output=True, text=True).stdout
    line = next(l for l in out.splitlines() if " -c " + unit + ".hip" in l)
    words = shlex.split(line.split(" 2> ")[0])
    return [w for w in words[:words.index("-o")] if not w.startswith("-Rpass")]


def digest(csrc, unit, llvm, tmp):
    obj = os.path.join(tmp, unit + ".dev")
    subprocess.run(compile_line(csrc, unit) + ["--cuda-device-only", "-o", obj], check=True, cwd=csrc,
                   stderr=subprocess.DEVNULL)
    elf = obj
    if open(obj, "rb").read(len(BUNDLE_MAGIC)) == BUNDLE_MAGIC:
        elf = os.path.join(tmp, unit + ".co")
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + obj,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + elf], check=True)
    h = hashlib.sha256()
    for tool in (["llvm-objdump", "-d"], ["llvm-readelf", "--notes"]):
        text = subprocess.run([os.path.join(llvm, tool[0])] + tool[1:] + [elf], check=True, capture_output=True,
                              text=True).stdout
        h.update("\n".join(l for l in text.splitlines() if elf not in l and os.path.basename(elf) not in l).encode())
    return h.hexdigest()[:32]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--csrc", default=os.path.join(ROOT, "pyopal_amd", "csrc"))
    ap.add_argument("--llvm", default="/opt/rocm/llvm/bin")
    ap.add_argument("--jobs", type=int, default=min(os.cpu_count() or 1, 8))
    ap.add_argument("units", nargs="*")
    args = ap.parse_args()
    csrc = os.path.abspath(args.csrc)
    units = args.units or units_of(csrc)
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        for unit, d in zip(units, pool.map(lambda u: digest(csrc, u, args.llvm, tmp), units)):
            print(unit, d, flush=True)


if __name__ == "__main__":
    sys.exit(main())
