#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libanerf_hip.so, kernel by kernel.

    python tools/isa_diff.py A.so B.so [--show N]

Each library's .hip_fatbin section holds one offload bundle per translation unit.  Every bundle is
unbundled (clang-offload-bundler), disassembled (llvm-objdump -d) and cut at the function labels; the
kernels' register, scratch and LDS figures come from the code objects' metadata notes.  Printed per kernel:
the instruction lines of A and B, whether they are identical, and any resource figure that differs.
Addresses and encodings are stripped, so a kernel that only moved compares equal; branch offsets and
pc-relative address literals are kept as they are, so a kernel whose distance to a constant table changed
(because another kernel of the unit grew or shrank) shows those lines.  Exit status 1 if anything differs.
--show N prints the first N differing lines of each differing kernel.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGICS = (b"__CLANG_OFFLOAD_BUNDLE__", b"CCOB")
RESOURCES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True).stdout


def code_objects(lib, tmp):
    """The gfx950 code objects of a library, one file per translation unit, in link order."""
    fat = os.path.join(tmp, "fatbin")
    run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, os.devnull)
    with open(fat, "rb") as f:
        blob = f.read()
    starts = sorted(m.start() for magic in MAGICS for m in re.finditer(re.escape(magic), blob))
    out = []
    for i, s in enumerate(starts):
        piece = os.path.join(tmp, f"bundle{i}")
        with open(piece, "wb") as f:
            f.write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        co = os.path.join(tmp, f"unit{i}.co")
        run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
            f"--input={piece}", f"--output={co}")
        out.append(co)
    return out


def functions(co):
    """{label: [instruction text, ...]} of one code object (addresses and encodings stripped)."""
    text = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co).decode()
    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            # (branch targets are printed as <label+0x..> offsets inside the function: position independent)
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return funcs


def resources(co):
    """{kernel: {resource: value}} from the amdhsa.kernels metadata note."""
    text = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).decode()
    res, cur = {}, {}
    for line in text.splitlines():  # (a kernel's own keys: "  - .key:" opens its record, "    .key:" continues it)
        m = re.match(r"^(  - |    )(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        first, key, val = m.groups()
        if first.strip():
            cur = {}
        if key in RESOURCES:
            cur[key] = val.strip()
        elif key == ".symbol":
            res[val.strip().strip("'")[:-len(".kd")]] = cur
    return res


def load(lib):
    with tempfile.TemporaryDirectory() as tmp:
        units = []
        for co in code_objects(lib, tmp):
            units.append((functions(co), resources(co)))
        return units


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--show", type=int, default=0)
    args = ap.parse_args()
    show = args.show
    a, b = load(args.a), load(args.b)
    if len(a) != len(b):
        sys.exit(f"{len(a)} code objects in A, {len(b)} in B")
    differ = 0
    for u, ((fa, ra), (fb, rb)) in enumerate(zip(a, b)):
        na, nb = sum(map(len, fa.values())), sum(map(len, fb.values()))
        print(f"== unit {u}: {len(fa)} / {len(fb)} functions, {na} / {nb} instruction lines")
        for name in sorted(set(fa) | set(fb)):
            la, lb = fa.get(name), fb.get(name)
            if la is None or lb is None:
                differ += 1
                print(f"  {'only in A' if lb is None else 'only in B'}: {len(la or lb)} lines  {name}")
                continue
            dr = {k: (ra.get(name, {}).get(k), rb.get(name, {}).get(k)) for k in RESOURCES
                  if ra.get(name, {}).get(k) != rb.get(name, {}).get(k)}
            same = la == lb
            if not same or dr:
                differ += 1
            rtxt = "".join(f" {k}: {x} -> {y}" for k, (x, y) in dr.items())
            print(f"  {'same' if same else 'DIFF'} {len(la)} {len(lb)}{rtxt}  {name}")
            if not same and show:
                d = [l for l in difflib.unified_diff(la, lb, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
                for l in d[:show]:
                    print("      " + l)
                print(f"      ({len(d)} changed lines)")
    print("no difference" if not differ else f"{differ} functions differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
