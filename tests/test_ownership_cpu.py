"""CPU-only: device memory has one owner.  Every allocation the library makes for itself goes through DevBuf (csrc/devbuf.h), which is what lets
mvrt_test_fail_allocation reach all of them (tests/test_gpu_alloc_failures.py); the only other hipMalloc / hipFree are the mvrt_malloc / mvrt_free
pass-throughs, which are the caller's memory."""
import os
import re

import massivevoxelraytracing_amd as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "massivevoxelraytracing_amd", "csrc")


def sources():
    out = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".h", ".hpp", ".cpp")):
            out[fn] = open(os.path.join(CSRC, fn)).read()
    assert {"api.hip", "svo_build.hip", "devbuf.h", "launch.h"} <= set(out)
    return out


def function_body(text, name):
    """the brace-matched body of the definition `name( ... ) { ... }`"""
    m = re.search(r"\b" + name + r"\s*\([^)]*\)\s*\{", text)
    assert m, name
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return m.end(), i


def test_hipmalloc_and_hipfree_only_in_devbuf_and_the_abi_pass_throughs():
    for fn, text in sources().items():
        if fn == "devbuf.h":
            assert text.count("hipMalloc(") == 1 and text.count("hipFree(") == 1
            continue
        if fn == "api.hip":  # cut the two pass-throughs out, each of which holds exactly its own call
            a0, a1 = function_body(text, "mvrt_malloc")
            assert text[a0:a1].count("hipMalloc(") == 1 and "hipFree(" not in text[a0:a1]
            text = text[:a0] + text[a1:]
            b0, b1 = function_body(text, "mvrt_free")
            assert text[b0:b1].count("hipFree(") == 1 and "hipMalloc(" not in text[b0:b1]
            text = text[:b0] + text[b1:]
        assert "hipMalloc(" not in text, fn
        assert "hipFree(" not in text, fn
        for other in ("hipMallocAsync", "hipFreeAsync", "hipMallocManaged", "hipMallocFromPoolAsync"):
            assert other not in text, (fn, other)


def test_no_hand_written_ownership_transfer_is_left():
    for fn, text in sources().items():
        assert "detach(" not in text, fn
        assert "freeLevels" not in text, fn
        assert not re.search(r"\bstruct\s+Buf\b", text), fn


def test_the_hook_entry_points_are_bound():
    lib = mv.lib()  # no GPU call: the tallies are plain counters, the hook a thread-local number
    assert len(mv.allocation_state()) == 3
    mv.set_test_fail_allocation(3)
    mv.set_test_fail_allocation(0)
    assert lib.mvrt_test_allocation_state(None, None, None) == 0
