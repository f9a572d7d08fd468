#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of librecstudio_amd.so, kernel for kernel.

    python tools/kernel_fingerprint.py OLD.so NEW.so

Per kernel: (vgpr, sgpr, agpr, scratch bytes, LDS bytes, code size, sha1 of the code bytes).  Prints every kernel that is in
one build only or whose tuple differs, then the two counts; the exit status is non-zero on any difference.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
NOTE = {"vgpr": ".vgpr_count", "sgpr": ".sgpr_count", "agpr": ".agpr_count", "scratch": ".private_segment_fixed_size",
        "lds": ".group_segment_fixed_size"}


def run(tool, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, tool), *args], cwd=cwd, check=True, capture_output=True, text=True).stdout


def code_object_kernels(path):
    """{kernel name: tuple} of one extracted code object"""
    meta, cur = {}, None          # the metadata note, printed as YAML: one "  - " block per kernel, its keys at depth 4
    for line in run("llvm-readelf", "--notes", path).splitlines():
        m = re.match(r"(  - |    )(\.\w+):\s+(.*)$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        cur[m.group(2)] = m.group(3).strip().strip("'")
        if m.group(2) == ".symbol":
            meta[cur[".symbol"][:-3]] = cur          # "<kernel>.kd"
    with tempfile.TemporaryDirectory() as tmp:
        text = os.path.join(tmp, "text.bin")
        run("llvm-objcopy", "-O", "binary", "--only-section=.text", path, text)
        blob = open(text, "rb").read()
    text_addr = None
    for line in run("llvm-readelf", "-S", "-W", path).splitlines():
        m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)", line)
        if m:
            text_addr = int(m.group(1), 16)
    out = {}
    for line in run("llvm-readelf", "-s", "-W", path).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[7] in meta:
            addr, size = int(f[1], 16) - text_addr, int(f[2], 0)
            k = meta[f[7]]
            out[f[7]] = tuple(int(k.get(NOTE[n], "0")) for n in ("vgpr", "sgpr", "agpr", "scratch", "lds")) + (
                size, hashlib.sha1(blob[addr:addr + size]).hexdigest())
    missing = set(meta) - set(out)
    if missing:
        sys.exit(f"{path}: no FUNC symbol for {sorted(missing)[:3]} ...")
    return out


def library_kernels(so):
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = os.path.join(tmp, "lib.so")
        os.symlink(os.path.abspath(so), lib)
        run("llvm-objdump", "--offloading", lib)      # writes one file per bundle entry next to its input
        for name in sorted(os.listdir(tmp)):
            if "gfx950" not in name:
                continue
            for k, v in code_object_kernels(os.path.join(tmp, name)).items():
                if k in kernels and kernels[k] != v:
                    sys.exit(f"{so}: kernel {k} appears twice with different code")
                kernels[k] = v
    if not kernels:
        sys.exit(f"{so}: no gfx950 kernels found")
    return kernels


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = library_kernels(sys.argv[1]), library_kernels(sys.argv[2])
    diffs = 0
    for k in sorted(set(old) | set(new)):
        if k not in new:
            print(f"only in {sys.argv[1]}: {k}")
        elif k not in old:
            print(f"only in {sys.argv[2]}: {k}")
        elif old[k] != new[k]:
            print(f"differs: {k}\n  old {old[k]}\n  new {new[k]}")
        else:
            continue
        diffs += 1
    print(f"{len(old)} kernels / {len(new)} kernels, {diffs} differing")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
