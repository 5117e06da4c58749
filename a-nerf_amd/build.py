"""Build libanerf_hip.so in-tree (hipcc, gfx950).  Used by __graft_entry__.build().

Rebuilds are content-addressed: a sha256 over the compiler command, every file under csrc/ and
include/anerf.h is stored next to the library (`libanerf_hip.so.stamp`).  A shipped binary whose
stamp does not match the sources is rebuilt, never reused because of its mtime.

The translation units compile in parallel into objects cached under `.objs/` by the hash of
their own dependencies (anerf_gemm.hip, anerf_step.hip, anerf_eval.hip, anerf_sequence.hip, anerf_posescore.hip and
anerf_prep.hip read only include/anerf.h; anerf_iso.hip, anerf_mesh.hip, anerf_raster.hip
and anerf_simplify.hip that and csrc/anerf_scan.hpp, which no other unit reads, anerf_iso.hip also its case table),
then link into the library: an edit of the training GEMMs, of the iso-surface, of the mesh, of the raster or of the
simplification kernels recompiles one unit, an edit of their shared scan header those four, never the render kernels'
instances.
The render kernels are two units over the same headers: anerf_render_f16.hip holds the fp16 instances of the three MLP
kernels and is the only unit compiled with RENDER_F16_FLAGS (MFMA results in VGPRs), anerf_render.hip everything else.
"""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
HEADER = os.path.join(os.path.dirname(HERE), "include", "anerf.h")
SRC = [os.path.join(CSRC, "anerf_render.hip"), os.path.join(CSRC, "anerf_render_f16.hip"),
       os.path.join(CSRC, "anerf_gemm.hip"),
       os.path.join(CSRC, "anerf_iso.hip"), os.path.join(CSRC, "anerf_mesh.hip"),
       os.path.join(CSRC, "anerf_raster.hip"), os.path.join(CSRC, "anerf_simplify.hip"),
       os.path.join(CSRC, "anerf_step.hip"), os.path.join(CSRC, "anerf_eval.hip"),
       os.path.join(CSRC, "anerf_sequence.hip"), os.path.join(CSRC, "anerf_posescore.hip"),
       os.path.join(CSRC, "anerf_prep.hip")]
# anerf_iso.hip's, anerf_mesh.hip's, anerf_raster.hip's and anerf_simplify.hip's alone
SCAN_HEADER = os.path.join(CSRC, "anerf_scan.hpp")
OUT = os.path.join(HERE, "libanerf_hip.so")
STAMP = OUT + ".stamp"
OBJS = os.path.join(HERE, ".objs")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-shared",
         "-Wno-unused-result"]
CFLAGS = [f for f in FLAGS if f != "-shared"]
# anerf_render_f16.hip alone: the fp16 layers' scale, relu and split run on the VALU, which cannot read AGPRs
# (tools/build_ab.sh and tools/build_stamps.sh compile that unit with the same option)
RENDER_F16_FLAGS = ["-mllvm", "-amdgpu-mfma-vgpr-form"]
UNIT_FLAGS = {"anerf_render_f16.hip": RENDER_F16_FLAGS}


def _hash(files, extra=""):
    h = hashlib.sha256()
    h.update((" ".join(FLAGS) + extra).encode())
    for name in sorted(UNIT_FLAGS):  # (of the units among `files`: every one for the library's stamp)
        if any(os.path.basename(d) == name for d in files):
            h.update((name + " " + " ".join(UNIT_FLAGS[name])).encode())
    for d in files:
        if os.path.isfile(d):
            h.update(os.path.basename(d).encode())
            with open(d, "rb") as f:
                h.update(f.read())
    return h.hexdigest()


def source_hash():
    """sha256 over the flags, the units' own flags and the bytes of csrc/* + include/anerf.h (sorted by name)."""
    deps = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC))
    deps.append(HEADER)
    return _hash(deps)


def unit_deps(src):
    """The files a translation unit reads: anerf_gemm.hip, anerf_step.hip, anerf_eval.hip, anerf_sequence.hip,
    anerf_posescore.hip and anerf_prep.hip only the C header; anerf_mesh.hip, anerf_raster.hip,
    anerf_simplify.hip and anerf_iso.hip the scan header and the C header, anerf_iso.hip its case table as well;
    anerf_render.hip and anerf_render_f16.hip every other csrc header."""
    name = os.path.basename(src)
    if name in ("anerf_gemm.hip", "anerf_step.hip", "anerf_eval.hip", "anerf_sequence.hip", "anerf_posescore.hip",
                "anerf_prep.hip"):
        return [src, HEADER]
    if name in ("anerf_mesh.hip", "anerf_raster.hip", "anerf_simplify.hip"):
        return [src, SCAN_HEADER, HEADER]
    if name == "anerf_iso.hip":
        return [src, os.path.join(CSRC, "anerf_iso_table.inc"), SCAN_HEADER, HEADER]
    return [src] + sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC)
                          if f.endswith(".hpp") and f != os.path.basename(SCAN_HEADER)) + [HEADER]


def stamp_matches():
    if not (os.path.exists(OUT) and os.path.exists(STAMP)):
        return False
    with open(STAMP) as f:
        return f.read().strip() == source_hash()


def _object(src, verbose, force=False):
    """The unit's cached object, compiled if its dependencies changed (discarded if they moved meanwhile)."""
    digest = _hash(unit_deps(src), "-c")
    name = os.path.splitext(os.path.basename(src))[0]
    obj = os.path.join(OBJS, f"{name}.{digest[:20]}.o")
    if os.path.exists(obj) and not force:
        return obj
    tmp = obj + ".tmp"
    cmd = [HIPCC] + CFLAGS + UNIT_FLAGS.get(os.path.basename(src), []) + ["-c", "-o", tmp, src]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    # hipcc reads the headers once per offload pass: a source edited during the build can give the host and
    # the device passes different struct layouts (a torn object).  Keep only an object whose inputs did not move
    if _hash(unit_deps(src), "-c") != digest:
        os.remove(tmp)
        raise RuntimeError(f"sources of {name} changed during the build: the object was discarded, build again")
    for old in os.listdir(OBJS):  # (one cached object per unit)
        if old.startswith(name + ".") and old.endswith(".o"):
            os.remove(os.path.join(OBJS, old))
    os.replace(tmp, obj)
    return obj


def build(force=False, verbose=True):
    if not force and stamp_matches():
        return OUT
    digest = source_hash()
    os.makedirs(OBJS, exist_ok=True)
    with ThreadPoolExecutor(max(1, len(SRC))) as ex:
        objs = list(ex.map(lambda s: _object(s, verbose, force), SRC))
    tmp = OUT + ".tmp"
    if os.path.exists(tmp):
        os.remove(tmp)
    cmd = [HIPCC] + FLAGS + ["-o", tmp] + objs
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    if source_hash() != digest:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise RuntimeError("sources changed during the build: the library was discarded, build again")
    # replace the library in one rename (a copy of the tree never sees a half-written file)
    os.replace(tmp, OUT)
    with open(STAMP, "w") as f:
        f.write(digest + "\n")
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
