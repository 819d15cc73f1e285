"""Write tests/golden/reference_pin_digests.json: a SHA-256 of every answer of the COMPILED reference (oracle/_ref/libmvrt_ref_walk.so and
libmvrt_ref_render.so; only answers free of sinf / cosf / atan2f / powf, which depend on the host's C library and are compared with the library alone) that
tests/test_reference_pins_cpu.py and tests/test_gpu_reference_pins.py compare against, so that those pins hold where oracle/_ref is absent.
Needs the reference tree (make -C oracle ref).  The CPU test module is run in recording mode -- it still compares the oracle with the library,
so a digest is only ever written for an answer the oracle reproduces or the run fails -- and the GPU build cases are answered directly."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import reference_pins as R  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    O.build()
    walk = R.load_walk(O, tree_decides=True)
    render = R.load_render(O, tree_decides=True)
    assert walk is not None and render is not None, "no compiled reference: the reference tree is needed"
    R._record = {}
    rc = pytest.main(["-q", "-x", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_reference_pins_cpu.py")])
    assert rc == 0, "the oracle differs from the compiled reference: nothing written"
    for key, tris, origin, dps, res, flags in R.class_build_cases() + R.mixed_build_cases():
        R._record[key] = R.digest(R.reference_build(walk, tris, origin, dps, res, flags))
    # the frames of tests/test_gpu_reference_pins.py, composed from the render and the walk library (no libm in them)
    sc = R.frame_scene(O)
    for name, cam in R.frame_cameras(sc).items():
        for W, H in R.PRIMARY_SIZES:
            R._record["render/primary/%s/%dx%d" % (name, W, H)] = R.digest(R.reference_primary((render, walk), sc, cam, W, H))
        R._record["render/first_hit/" + name] = R.digest(R.reference_first_hit((render, walk), O, sc, cam))
    with open(R.DIGESTS, "w") as f:
        json.dump(dict(sorted(R._record.items())), f, indent=0)
        f.write("\n")
    print(len(R._record), "digests ->", R.DIGESTS)


if __name__ == "__main__":
    main()
