"""Code-object metadata of the kernels in compiled objects, and a comparison of two builds:
  python3 tools/kernel_resource_usage.py OBJ_DIR [OTHER_OBJ_DIR] [--match SUBSTRING ...] [--files GLOB ...]
Per kernel of every matching object under OBJ_DIR (a csrc/.obj directory): VGPRs, AGPRs, SGPRs, spilled VGPRs / SGPRs, scratch
(private segment) bytes, static LDS bytes and code size, read from the gfx950 code object inside the object file (the
.hip_fatbin section, unbundled; llvm-readelf --notes for the metadata, the symbol table for the size).  With OTHER_OBJ_DIR the same
for that build and one line per kernel saying whether every figure is equal.  Needs no GPU."""
import argparse
import fnmatch
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
KEYS = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("vgpr_spill", ".vgpr_spill_count"),
        ("sgpr_spill", ".sgpr_spill_count"), ("scratch", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size"))


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels_of(obj):
    """{kernel symbol: {figure: value}} of one object file"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
        run(os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
        if not os.path.exists(fat) or not os.path.getsize(fat):
            return {}
        run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co)
        notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
        syms = run(os.path.join(LLVM, "llvm-readelf"), "-sW", co)
    sizes = {m.group(2): int(m.group(1)) for m in re.finditer(r"^\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)$", syms, re.M)}
    out = {}
    for block in re.split(r"^\s+- \.agpr_count:", notes, flags=re.M)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        figs = {k: int(re.search(re.escape(key) + r":\s+(\d+)", block).group(1)) for k, key in KEYS}
        figs["code_bytes"] = sizes.get(name.group(1), -1)
        out[name.group(1)] = figs
    return out


def collect(obj_dir, globs, match):
    out = {}
    for fn in sorted(os.listdir(obj_dir)):
        if fn.endswith(".o") and any(fnmatch.fnmatch(fn, g) for g in globs):
            for k, figs in kernels_of(os.path.join(obj_dir, fn)).items():
                if not match or any(m in k for m in match):
                    out[(fn, k)] = figs
    return out


def line(figs):
    return "  ".join("%s=%d" % (k, figs[k]) for k in [k for k, _ in KEYS] + ["code_bytes"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("obj_dir")
    ap.add_argument("other", nargs="?")
    ap.add_argument("--match", nargs="*", default=[])
    ap.add_argument("--files", nargs="*", default=["*.o"])
    args = ap.parse_args()
    a = collect(args.obj_dir, args.files, args.match)
    b = collect(args.other, args.files, args.match) if args.other else None
    differ = 0
    for key in sorted(set(a) | set(b or {})):
        print("%s  %s" % key)
        if key in a:
            print("    %s%s" % ("first:  " if b is not None else "", line(a[key])))
        if b is not None:
            if key in b:
                print("    second: %s" % line(b[key]))
            verdict = "EQUAL" if a.get(key) == b.get(key) else "only in the %s build" % ("first" if key in a else "second") if (key in a) != (key in b) else "DIFFERENT"
            differ += verdict == "DIFFERENT"
            print("    -> %s" % verdict)
    if b is not None:
        print("%d kernel(s) in both builds, %d differ" % (len(set(a) & set(b)), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
