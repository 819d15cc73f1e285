"""What the tests of the applications (apps/voxel_mesh in tests/test_gpu_*_app.py; apps/rtcamp_batch, apps/device_render) share: the program and a run of it, small
triangle meshes in voxel units, the OBJ writers and the readers of the images the applications write."""
import os
import struct
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "apps", "voxel_mesh")


def run(*args):
    out = subprocess.check_output([APP] + [str(a) for a in args], timeout=120).decode()
    print(out)
    return out


def write_obj(path, v, colours=None):
    """v: (n, 3, 3) triangles or their (3 n, 3) vertices; colours: None or one (r, g, b) per vertex, written behind its position"""
    v = np.asarray(v).reshape(-1, 3)
    rows = v if colours is None else [tuple(p) + tuple(q) for p, q in zip(v, colours)]
    fmt = "v" + " %.9g" * (3 if colours is None else 6) + "\n"
    with open(path, "w") as f:
        f.write("".join(fmt % tuple(r) for r in rows) + "".join("f %d %d %d\n" % (3 * t + 1, 3 * t + 2, 3 * t + 3) for t in range(len(v) // 3)))
    return str(path)


def write_reader_obj(path, tris, with_colors=False):
    """the same mesh in the forms an OBJ reader has to take: a comment line, relative indices on every other face and v//vn on the rest"""
    v = tris.reshape(-1, 3)
    with open(path, "w") as f:
        f.write("# test mesh\n")
        for i, p in enumerate(v):
            if with_colors:
                f.write("v %.9g %.9g %.9g %.3f %.3f %.3f\n" % (p[0], p[1], p[2], (i % 7) / 7.0, (i % 5) / 5.0, (i % 3) / 3.0))
            else:
                f.write("v %.9g %.9g %.9g\n" % tuple(p))
        for t in range(len(v) // 3):
            if t % 2:
                f.write("f %d//%d %d//%d %d//%d\n" % (3 * t + 1, 1, 3 * t + 2, 1, 3 * t + 3, 1))
            else:
                f.write("f %d %d %d\n" % (3 * t + 1 - len(v) - 1, 3 * t + 2 - len(v) - 1, 3 * t + 3 - len(v) - 1))  # relative indices


def run_app(exe, args):
    r = subprocess.run(["timeout", "-k", "10", "120", exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def read_ppm(path, W, H):
    data = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (W, H)
    assert data.startswith(head), data[:32]
    return np.frombuffer(data[len(head):], np.uint8).reshape(W * H, 3)


def read_png_rgba(path):
    d = open(path, "rb").read()
    assert d[:8] == b"\x89PNG\r\n\x1a\n", d[:8]
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(d):
        n, typ = struct.unpack(">I4s", d[pos:pos + 8])
        body = d[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", d[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(typ + body) & 0xFFFFFFFF, ("crc", typ)
        if typ == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            assert (depth, ctype) == (8, 6), (depth, ctype)
        elif typ == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w * 4 + 1)
    assert (raw[:, 0] == 0).all(), "a filtered row"
    return raw[:, 1:].reshape(h, w, 4)


def quad(a, b, c, d):
    return [a, b, c, a, c, d]


def slab(x0, x1, y0, y1, z):
    return quad((x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z))


def block(lo, hi):
    """horizontal slabs through the middle of the layers z = lo .. hi - 1: a solid block of (hi - lo)^3 voxels at [lo, hi)^3, in voxel units"""
    v = []
    for k in range(lo, hi):
        v += slab(lo + 0.25, hi - 0.25, lo + 0.25, hi - 0.25, k + 0.5)
    return v


def corners(lo, hi, d):
    """two small triangles that stretch the bounding grid to [lo, hi]^3"""
    return [(lo, lo, lo), (lo + d, lo, lo), (lo, lo + d, lo), (hi, hi, hi), (hi - d, hi, hi), (hi, hi - d, hi)]


def holed_box():
    """the unit cube as triangles; its floor z = 0 is four rectangles around the hole [0.43, 0.51]^2.  Two small triangles off two opposite corners stretch the
    bounding grid to [-0.03, 1.03]^3, so that no face lies on a cell boundary: the floor voxel x = y = 7 of the 16^3 grid spans [0.43375, 0.5], inside the hole,
    and its neighbours 6 and 8 reach under the rectangles"""
    v = [(-0.03, -0.03, -0.03), (-0.02, -0.03, -0.03), (-0.03, -0.02, -0.03), (1.03, 1.03, 1.03), (1.02, 1.03, 1.03), (1.03, 1.02, 1.03)]
    for axis in range(3):
        for side in (0.0, 1.0):
            if axis == 2 and side == 0.0:
                continue
            p = [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]
            v += quad(*[tuple(np.insert(np.array(q), axis, side)) for q in p])
    h0, h1 = 0.43, 0.51
    for (x0, x1, y0, y1) in ((0.0, 1.0, 0.0, h0), (0.0, 1.0, h1, 1.0), (0.0, h0, h0, h1), (h1, 1.0, h0, h1)):
        v += quad((x0, y0, 0.0), (x1, y0, 0.0), (x1, y1, 0.0), (x0, y1, 0.0))
    return np.array(v, np.float32).reshape(-1, 3, 3)
