"""The arithmetic of the surface smoothing without a GPU: csrc/smooth_rule.h (the rounded division, the step with its clamp count, the slot of a quad edge,
the position of a displaced corner) and the corner tables of csrc/surface_weld.h against floor arithmetic in int64 and long double.  tests/hip/smooth_host.hip
is a program of its own that makes no HIP call; it is compiled for the host with hipcc and run here, once plainly and once under the address and
undefined-behaviour sanitizers."""
import os

import pytest

import common


@pytest.mark.skipif(not os.path.exists(common.HIPCC), reason="no hipcc")
@pytest.mark.parametrize("sanitize", [False, True])
def test_smooth_rule_against_floor_arithmetic(tmp_path, sanitize):
    common.run_host_probe(tmp_path, "smooth_host", "smooth host checks ok", sanitize=sanitize, timeout=300)
