"""Fixture for the mesh normals (tests/test_mesh_attrs.py): the REFERENCE viewer's per-vertex normals on the
checker's meshes.

Build container only (reads the reference tree like make_golden.py; the fixture it writes is committed, the GPU
box never runs this).  The reference's viewer shades an extracted mesh with normals it accumulates from the faces
on the host (render_mesh.py:35-53, compute_normal / normalize_v3).  Those two functions are read out of the
reference's file when this runs -- its module cannot be imported without a display, and nothing of it is copied
here -- and applied to the isosurface_reference meshes of four analytic fields of tests/_iso_cases.py.  The result,
face-accumulated normals only (the meshes are recomputed by the test), goes to tests/golden/mesh_normals_ref.npz.

Usage:  python tests/golden/make_mesh_normals_golden.py [reference directory]
"""
import ast
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))

iso = importlib.import_module("a-nerf_amd.isosurface")

FIELDS = {"sphere_field": 0.0, "torus_field": 0.0, "two_spheres_field": 0.0, "blobs_field": 0.5}  # name: threshold


def reference_functions(ref_dir):
    """compute_normal of the reference's render_mesh.py (with the normalize_v3 it calls), compiled from the
    file's own text: only these two function definitions are executed."""
    path = os.path.join(ref_dir, "render_mesh.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    want = ("normalize_v3", "compute_normal")
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert sorted(d.name for d in defs) == sorted(want), f"{path}: {want} not found"
    ns = {"np": np}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns["compute_normal"]


def main(ref_dir):
    import _iso_cases as C
    compute_normal = reference_functions(ref_dir)
    out = {}
    for name, thr in FIELDS.items():
        v, t = iso.isosurface_reference(getattr(C, name)(), thr)
        n = compute_normal(v.astype(np.float32).copy(), t.astype(np.int64))
        assert n.shape == v.shape and np.isfinite(n).all()
        out[name] = n.astype(np.float32)
        out[name + "_threshold"] = np.float32(thr)
        print(f"{name}: {len(v)} vertices, {len(t)} triangles")
    path = os.path.join(HERE, "mesh_normals_ref.npz")
    np.savez_compressed(path, meta=np.array(repr(dict(source="render_mesh.py:35-53 compute_normal on "
                                                             "isosurface_reference(field, threshold)",
                                                      fields=FIELDS))), **out)
    print(f"wrote {path}: {sum(len(out[k]) for k in FIELDS)} rows, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    import make_golden as mg
    main(sys.argv[1] if len(sys.argv) > 1 else mg.REF)
