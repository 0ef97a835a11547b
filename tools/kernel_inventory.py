#!/usr/bin/env python3
"""Inventory of the device kernels inside a built libhbmpc_hip.so.

One sorted line per kernel: mangled name, .vgpr_count, .sgpr_count, .private_segment_fixed_size, .group_segment_fixed_size,
size of its text in bytes.  Two builds whose inventories are equal hold the same set of kernels with the same resources: a
refactor of the host side diffs the two outputs and expects nothing.

    python3 tools/kernel_inventory.py mpc-protocols_amd/libhbmpc_hip.so > inventory.txt
    python3 tools/kernel_inventory.py --per-object mpc-protocols_amd/libhbmpc_hip.so
        # kernels per code object, in link order.  An object file without device code embeds none: when the count of code
        # objects equals the count of csrc/tu_*.hip, hbmpc_capi.o and capi_pipelines.o hold host code only
    python3 tools/kernel_inventory.py --disasm-dir out/ --match 'k_binop|k_scalarop' mpc-protocols_amd/libhbmpc_hip.so

--disasm-dir writes one file per kernel (named by the SHA-1 of the mangled name, listed in INDEX.txt) with the kernel's
instructions, addresses and encodings dropped, so that two builds compare with `diff -r`.

Standard library plus llvm-objdump / llvm-readelf (LLVM_BIN, default /opt/rocm/llvm/bin).  The code objects are taken out of
the file with `llvm-objdump --offloading`, which writes next to its input: the input is copied to a temporary directory first.
A kernel name found in several code objects with differing numbers is an error (exit status 1).
"""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM_BIN = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM_BIN, name), *args], check=True, capture_output=True, text=True).stdout


def code_objects(path, arch, tmp):
    """The gfx950 code objects of `path`, in the order of the bundles (the link order of the object files)."""
    local = os.path.join(tmp, os.path.basename(path))
    shutil.copy(path, local)
    tool("llvm-objdump", "--offloading", local)
    found = []
    for f in os.listdir(tmp):
        m = re.match(re.escape(os.path.basename(path)) + r"\.(\d+)\.hip.*-" + re.escape(arch) + "$", f)
        if m and os.path.getsize(os.path.join(tmp, f)):
            found.append((int(m.group(1)), os.path.join(tmp, f)))
    return sorted(found)


def kernels_of(co):
    """{mangled name: (vgpr, sgpr, private, group, text bytes)} of one code object."""
    sizes = {}
    for line in tool("llvm-readelf", "-s", "-W", "--symbols", co).splitlines():
        p = line.split()
        if len(p) == 8 and p[3] == "FUNC":
            sizes[p[7]] = int(p[2])
    out = {}
    # the metadata note is YAML; each kernel is one "  - " item of amdhsa.kernels with its scalar fields at four spaces
    notes = tool("llvm-readelf", "--notes", co)
    section = notes.split("amdhsa.kernels:", 1)[1].split("\namdhsa.", 1)[0] if "amdhsa.kernels:" in notes else ""
    for item in re.split(r"^  - ", section, flags=re.M)[1:]:
        kv = dict(re.findall(r"^(?:    )?(\.\w+): +(\S+)$", item, flags=re.M))
        name = kv[".name"]
        out[name] = tuple(int(kv[f]) for f in FIELDS) + (sizes[name],)
    return out


def disassembly(co):
    """{symbol: [instruction, ...]} of one code object, without addresses and encodings."""
    out, cur = {}, None
    for line in tool("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^<(.+)>:$", line.strip())
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip() and line.strip() != "...":  # "...": zero bytes that pad the end of a function
            cur.append(re.sub(r"\s*//.*$", "", line.strip()))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("library")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--per-object", action="store_true", help="print the number of kernels of each code object instead")
    ap.add_argument("--disasm-dir", help="write the kernels' instructions here, one file per kernel")
    ap.add_argument("--match", default="", help="with --disasm-dir: only kernels whose mangled name matches this regex")
    a = ap.parse_args()
    merged, bad, index = {}, 0, set()
    with tempfile.TemporaryDirectory() as tmp:
        cos = code_objects(a.library, a.arch, tmp)
        if not cos:
            sys.exit(f"no {a.arch} code object in {a.library}")
        for idx, co in cos:
            ks = kernels_of(co)
            if a.per_object:
                print(f"code object {idx}: {len(ks)} kernels")
            for name, v in ks.items():
                if merged.setdefault(name, v) != v:
                    print(f"{name}: {merged[name]} and {v} in different code objects", file=sys.stderr)
                    bad += 1
            if a.disasm_dir:
                os.makedirs(a.disasm_dir, exist_ok=True)
                dis = disassembly(co)
                for name in ks:
                    if re.search(a.match, name):
                        with open(os.path.join(a.disasm_dir, hashlib.sha1(name.encode()).hexdigest() + ".s"), "w") as f:
                            f.write("\n".join(dis[name]) + "\n")
                        index.add(name)
    if a.disasm_dir:
        with open(os.path.join(a.disasm_dir, "INDEX.txt"), "w") as f:
            f.writelines(f"{hashlib.sha1(n.encode()).hexdigest()} {n}\n" for n in sorted(index))
    if not a.per_object:
        for name in sorted(merged):
            print(name, *merged[name])
    print(f"{len(merged)} kernels in {len(cos)} code objects", file=sys.stderr)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
