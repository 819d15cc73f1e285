#!/usr/bin/env python3
"""Regenerate the DATA fixtures under tests/golden/ from the reference's data files.

Run in the build container only (reads /root/reference; the GPU box has no reference tree).
Fixtures are data, never source: the triangle soup of scenes/bunny.obj as raw float32, a
byte copy of the 8 KB environment map bin/monks_forest_s.hdr, and the answers of the reference's
MurmurHash3.cpp / morton.hpp (through oracle/_ref, built by `make -C oracle ref`) to the inputs of
tests/test_oracle_pins.py, as raw little-endian uint32 / uint64.
"""
import hashlib, os, shutil, sys
import numpy as np

REF = os.environ.get("MVRT_REFERENCE", "/root/reference")
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden")


def load_obj_triangles(path):
    verts, tris = [], []
    with open(path) as f:
        for line in f:
            if line.startswith("v "):
                verts.append([float(x) for x in line.split()[1:4]])
            elif line.startswith("f "):
                idx = [int(tok.split("/")[0]) for tok in line.split()[1:]]
                for k in range(1, len(idx) - 1):  # fan
                    tris.append([idx[0] - 1, idx[k] - 1, idx[k + 1] - 1])
    v = np.asarray(verts, dtype=np.float32)
    t = np.asarray(tris, dtype=np.int64)
    return v[t].reshape(-1, 9)  # nTri x (v0 v1 v2)


def ref_vectors():
    """the reference's murmur hashes and morton codes of the pins' inputs (tests/common.py)"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import common
    from oracle import oracle as O
    ref = O.load_ref()
    if ref is None:
        sys.exit("oracle/_ref is not built: make -C oracle ref")
    h = np.array([ref.ref_murmur3_x86_32(xs.ctypes.data, len(xs), s) for xs, s in common.murmur_cases()], np.uint32)
    h.astype("<u4").tofile(os.path.join(OUT, common.REF_MURMUR_U32))
    xyz = np.ascontiguousarray(common.morton_points()[:common.REF_MORTON_STORED])
    a, b, c = (np.zeros(len(xyz), np.uint64) for _ in range(3))
    ref.ref_morton_batch(xyz.ctypes.data, len(xyz), a.ctypes.data, b.ctypes.data, c.ctypes.data)
    assert (a == b).all() and (a == c).all()
    a.astype("<u8").tofile(os.path.join(OUT, common.REF_MORTON_U64))
    return [common.REF_MURMUR_U32, common.REF_MORTON_U64]


def main():
    os.makedirs(OUT, exist_ok=True)
    tri = load_obj_triangles(os.path.join(REF, "scenes", "bunny.obj"))
    tri.astype("<f4").tofile(os.path.join(OUT, "bunny_tris.f32"))
    shutil.copyfile(os.path.join(REF, "bin", "monks_forest_s.hdr"), os.path.join(OUT, "monks_forest_s.hdr"))
    for name in ["bunny_tris.f32", "monks_forest_s.hdr"] + ref_vectors():
        p = os.path.join(OUT, name)
        print(name, os.path.getsize(p), hashlib.sha256(open(p, "rb").read()).hexdigest())
    print("triangles", tri.shape[0], "bbox", tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0))


if __name__ == "__main__":
    sys.exit(main())
