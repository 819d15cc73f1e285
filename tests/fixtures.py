"""The module-scoped fixtures that the test files share.  A test file imports the ones it names in its tests' arguments (`from fixtures import O, mv  # noqa: F401`);
hdr and bunny256 ask for O, so a file that imports them imports O with them.  tests/common.py stays free of pytest: __graft_entry__.smoke() imports it."""
import pytest

from common import bunny_tris, hdr_bytes


def load():
    """the package with its library loaded, for whatever runs without a device"""
    import massivevoxelraytracing_amd as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def mv():
    m = load()
    assert m.device_count() >= 1
    return m


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def hdr(O):
    return O.decode_rgbe(hdr_bytes())


@pytest.fixture(scope="module")
def bunny256(O):
    return O.build_scene_from_triangles(bunny_tris(), 256)
