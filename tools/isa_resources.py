"""Static resource figures of gfx950 kernels: vector registers, scratch bytes and the number of VECTOR INSTRUCTIONS, one line
per kernel (tools/kernel_resource_usage.py compares the descriptors of two object directories; this one counts instructions, which
is what an issue-bound kernel's time follows).  Two sources:

  an assembly listing (hipcc -S --cuda-device-only, or the .s of -save-temps):
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include -S --cuda-device-only -o q.s near-light-client_amd/csrc/prover_kernels.hip
    python tools/isa_resources.py q.s [name-substring ...]

  the built library (its code objects are unbundled into a temporary directory and disassembled; needs ROCm's llvm tools):
    python tools/isa_resources.py near-light-client_amd/libnlx.so [name-substring ...]
  A kernel that calls non-inlined device functions (the generated AIR kernels: one function per program segment) is listed with
  the vector instructions of its own body AND of every function of its code object; its register count covers its callees.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")


def kernels(text):
    """{symbol: dict(vgpr, agpr, scratch, occupancy, valu, total)} from a listing's bodies and its resource comments"""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)", text):
        name = m.group(1)
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), text, re.S | re.M)
        lines = [ln.split(";")[0].strip() for ln in body.group(1).splitlines()] if body else []
        ins = [ln for ln in lines if ln and not ln.startswith(".") and not ln.endswith(":")]
        d = {"valu": sum(1 for ln in ins if ln.startswith("v_")), "total": len(ins)}
        for key, pat in (("vgpr", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
                         ("occupancy", r"; Occupancy: (\d+)")):
            mm = re.search(r"^%s:[^\n]*\n.*?%s" % (re.escape(name), pat), text, re.S | re.M)
            d[key] = int(mm.group(1)) if mm else -1
        out[name] = d
    return out


def library_kernels(lib):
    """[(kernel symbol, dict(vgpr, agpr, scratch, valu, valu_object, functions))] of every code object bundled in `lib`"""
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "lib.so")
        os.symlink(os.path.abspath(lib), local)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], check=True, capture_output=True, cwd=tmp)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            co = os.path.join(tmp, f)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                                 text=True).stdout
            valu, cur = {}, None
            for ln in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
                if m:
                    cur = m.group(1)
                    valu[cur] = 0
                elif cur is not None and ln.strip().startswith("v_"):
                    valu[cur] += 1
            for blk in notes.split("- .agpr_count:")[1:]:
                get = lambda key: re.search(r"\.%s:\s+(\S+)" % key, blk)
                name = get("name").group(1)
                rows.append((name, {"agpr": int(blk.split()[0]), "vgpr": int(get("vgpr_count").group(1)),
                                    "scratch": int(get("private_segment_fixed_size").group(1)), "valu": valu.get(name, -1),
                                    "valu_object": sum(valu.values()), "functions": len(valu)}))
    return rows


if __name__ == "__main__":
    want = sys.argv[2:]
    if sys.argv[1].endswith(".so"):
        for name, d in sorted(library_kernels(sys.argv[1])):
            if want and not any(w in name for w in want):
                continue
            print("%-72s vgpr %3d agpr %3d scratch %5d vector-instructions %6d (code object: %7d in %3d functions)" %
                  (name[:72], d["vgpr"], d["agpr"], d["scratch"], d["valu"], d["valu_object"], d["functions"]))
    else:
        ks = kernels(open(sys.argv[1]).read())
        for name in sorted(ks):
            if want and not any(w in name for w in want):
                continue
            d = ks[name]
            print("%-72s vgpr %3d agpr %3d scratch %5d occupancy %d vector-instructions %6d of %6d" %
                  (name[:72], d["vgpr"], d["agpr"], d["scratch"], d["occupancy"], d["valu"], d["total"]))
