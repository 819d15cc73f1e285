"""What the stream-order tests (tests/test_gpu_stream_order.py) share: tests/hip/stream_hold.hip compiled with hipcc and called through ctypes -- a non-blocking
stream and a bounded kernel that keeps a stream busy -- the window around it, the asynchronous copy that plays the producer, the read-back that waits for one
stream only, and the calibration that finds a created stream which does not share a hardware queue with the default stream."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCE = os.path.join(ROOT, "tests", "hip", "stream_hold.hip")

MAX_HOLD_MS = 250  # SH_MAX_MS of stream_hold.hip: sh_hold clamps to it
CALIBRATION_HOLD_MS = 40
# The hold has to outlast the host time from entering a call to the library's first device operation.  Measured on an MI355X with the library as it was before
# this file existed: every case's whole call, timed on the default stream with nothing held (its first device operation comes earlier still).  The longest was
# a path tracer set up from nothing, 12.6 ms (31.4 ms the first time, with the code objects to load); the longest call with device inputs, the kind regime C
# is about, took 2.5 ms.  The hold is ten times the longest.  test_gpu_stream_order.py times the same calls on every run and prints them (CALL_MS): that line
# is what to read before changing these two numbers.
MEASURED_CALL_MS = 12.6
HOLD_MS = 126  # 10 x MEASURED_CALL_MS, below MAX_HOLD_MS


def compile_hold(out_dir):
    """tests/hip/stream_hold.hip as a shared library, built the way rays.compile_probe builds its probes"""
    so = os.path.join(str(out_dir), "stream_hold.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", SOURCE, "-o", so], timeout=300)
    return so


def load_hold(so):
    lib = C.CDLL(so)
    lib.sh_stream_create_nonblocking.restype = C.c_int
    lib.sh_stream_create_nonblocking.argtypes = [C.c_void_p]
    lib.sh_stream_destroy.restype = C.c_int
    lib.sh_stream_destroy.argtypes = [C.c_void_p]
    lib.sh_hold.restype = C.c_int
    lib.sh_hold.argtypes = [C.c_void_p, C.c_uint32]
    return lib


class Streams:
    """the loaded helper, the package and the calibrated stream S (a raw hipStream_t as an int; None is the default stream)"""

    def __init__(self, mv, lib):
        self.mv, self.lib, self.S, self.report = mv, lib, None, []

    def create(self):
        s = C.c_void_p(0)
        rc = self.lib.sh_stream_create_nonblocking(C.byref(s))
        assert rc == 0 and s.value, "hipStreamCreateWithFlags( hipStreamNonBlocking ) failed: %d" % rc
        return s.value

    def destroy(self, s):
        assert self.lib.sh_stream_destroy(s) == 0

    def sync(self, stream):
        rc = self.mv.lib().mvrt_stream_synchronize(stream)
        assert rc == 0, self.mv.lib().mvrt_last_error()

    def hold(self, stream, ms):
        rc = self.lib.sh_hold(stream, int(ms))
        assert rc == 0, "sh_hold: HIP error %d" % rc

    def held(self, stream, ms=None):
        return Held(self, stream, HOLD_MS if ms is None else ms)

    def async_fill(self, dst, src, stream):
        """mvrt_memcpy_d2d, the one copy the header documents as asynchronous: the producer of the tests"""
        assert dst.nbytes == src.nbytes
        if dst.nbytes:
            self.mv.memcpy_d2d(dst, src, dst.nbytes, stream)

    def snapshot(self, devs, stream):
        """device arrays -> host arrays through fresh device arrays filled on `stream`; only `stream` is waited for, never the device"""
        copies = [self.mv.DeviceArray(d.shape, d.dtype) for d in devs]
        for c, d in zip(copies, devs):
            self.async_fill(c, d, stream)
        self.sync(stream)
        out = [c.to_host() for c in copies]  # (to_host waits for the default stream: callers are past their window's last queued operation here)
        return out, copies  # the copies go back to the caller: freeing device memory waits for the whole device, so it is done outside the window


class Held:
    """with Held(streams, stream, ms): the stream is busy for ms milliseconds from here on; on exit the held stream is synchronised"""

    def __init__(self, streams, stream, ms):
        self.streams, self.stream, self.ms = streams, stream, ms

    def __enter__(self):
        self.streams.hold(self.stream, self.ms)
        return self

    def __exit__(self, *exc):
        self.streams.sync(self.stream)
        return False


def _timed_copy_while_held(st, held_stream, copy_stream, word, host):
    """hold one stream, make a 4-byte host-to-device copy on the other (it waits for that other stream alone) and time the copy on the host"""
    st.hold(held_stream, CALIBRATION_HOLD_MS)
    t0 = time.perf_counter()
    rc = st.mv.lib().mvrt_memcpy_h2d(word.ptr, host.ctypes.data_as(C.c_void_p), 4, copy_stream)
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0
    t0 = time.perf_counter()
    st.sync(held_stream)
    return ms, ms + (time.perf_counter() - t0) * 1e3


def calibrate(st, tries=4):
    """S = the first created non-blocking stream on which a hold does not stall the default stream, nor a hold on the default stream it.  Without one the hold
    would hide every mis-ordering, so this fails and says what was timed."""
    word, host = st.mv.DeviceArray(1, np.uint32), np.zeros(1, np.uint32)
    st.hold(None, 1)  # the first launch loads the code object: kept out of the timings
    st.sync(None)
    for k in range(tries):
        s = st.create()
        a, a_all = _timed_copy_while_held(st, s, None, word, host)
        b, b_all = _timed_copy_while_held(st, None, s, word, host)
        st.report.append({"stream": k, "default_copy_ms_while_S_held": round(a, 3), "S_copy_ms_while_default_held": round(b, 3),
                          "hold_ms_seen_from_host": [round(a_all, 3), round(b_all, 3)]})
        if a < CALIBRATION_HOLD_MS / 2 and b < CALIBRATION_HOLD_MS / 2 and min(a_all, b_all) >= CALIBRATION_HOLD_MS / 2:
            st.S = s
            return st
        st.destroy(s)
    pytest.fail("stream calibration: none of %d non-blocking streams ran beside the default stream.  Timed on the host: a 4-byte mvrt_memcpy_h2d on one stream "
                "while a %d ms hold kernel ran on the other (must return in under %d ms), and the hold as the host saw it (copy plus the wait for the held "
                "stream, at least %d ms): %r" % (tries, CALIBRATION_HOLD_MS, CALIBRATION_HOLD_MS // 2, CALIBRATION_HOLD_MS // 2, st.report))


@pytest.fixture(scope="module")
def streams(tmp_path_factory):
    from fixtures import load
    mv = load()
    assert mv.device_count() >= 1
    st = calibrate(Streams(mv, load_hold(compile_hold(tmp_path_factory.mktemp("stream_hold")))))
    print("stream calibration:", st.report)
    yield st
    mv.synchronize()
    st.destroy(st.S)
