"""The device-resident log reader (include/nvl_framing.h: nvl_log_read_dev;
kernels nvlevelz_amd/csrc/crc32c_log_read.hip; nvl::shims::DeviceLogReader),
GPU side.

Parity anchors:
* tests/golden/log_cases.json -- the REFERENCE's log::Reader traces: every
  case through DeviceLogReader (tests/native/log_read_harness.cc);
* nvl_log_read(..., NVL_FRAMING_HOST), itself anchored to the reference's
  traces without a GPU (tests/test_log_read.py): nvl_log_read_dev must return
  exactly its totals, records, reports and payload bytes on the fixtures'
  images, the record-level edge images at every allocation shift, the header
  fuzz images of tests/test_log_scan_dev.py, dense images that put a breaking
  event next to every tile edge of the kernels' scans, images built around
  the gather's paths, and with the scan's window forced to 1 and 3 blocks
  (NVL_LOG_DEV_WINDOW_BLOCKS, one child process each).

Run as a script (the window children): `python tests/test_log_read_dev.py`
checks the edge, seam and gather images under the environment's window size.
"""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import log_read_cases as lrc  # noqa: E402
from test_log_scan_dev import _device_copy, fixture_images, fuzz_image, gpu_present, shim  # noqa: E402,F401

NATIVE = os.path.join(ROOT, "tests", "native")


def _lib():
    from nvlevelz_amd import _lib as L
    return L


def _need_gpu():
    if not gpu_present():
        pytest.skip("no GPU")


def check_identity(L, img, initial_offset, checksum, what, shift=0, stream=None, payload_shift=0):
    """nvl_log_read_dev == nvl_log_read(NVL_FRAMING_HOST), with the payload in
    device and in host memory; returns the host result."""
    import torch
    want = lrc.host_read(L, img, initial_offset, checksum)
    d = _device_copy(img, shift)
    torch.cuda.synchronize()
    for host_payload in (False, True):
        got = lrc.dev_read(L, d, len(img), initial_offset, checksum, stream, want[0], host_payload, payload_shift)
        assert got == want, (what, shift, host_payload, lrc.describe(got), lrc.describe(want))
    return want


def seam_images():
    """(name, image): the unbroken dense record and one breaking event of each
    kind next to every edge of 64, 256 and 1024 events."""
    img, n = lrc.dense_image()
    assert n > 10000
    yield "dense", img
    for at in lrc.seam_positions():
        for breaker in ("bad", "full", "unknown"):
            yield f"dense_{breaker}_{at}", lrc.dense_image(breaker, at)[0]


def run_edge_seam_gather(L, shifts=(0,)):
    """Everything the window children check; returns (records, reports, fragments of the longest record)."""
    import numpy as np
    nrec = nrep = longest = 0

    def note(want):
        nonlocal nrec, nrep, longest
        nrec += want[0][0]
        nrep += want[0][1]
        if want[0][0]:
            longest = max(longest, int(np.frombuffer(want[1], dtype="<u4").reshape(-1, 8)[:, 6].max()))

    for name, img, initial_offset, checksum in lrc.edge_cases():
        for shift in shifts:
            note(check_identity(L, img, initial_offset, checksum, name, shift))
    for name, img in seam_images():
        note(check_identity(L, img, 0, 1, name, 1))
    for pre in (1, 2, 3):
        note(check_identity(L, lrc.gather_image(pre), 0, 1, ("gather", pre), pre, payload_shift=pre - 1))
    return nrec, nrep, longest


@pytest.fixture(scope="module")
def L():
    return _lib()


@pytest.fixture(scope="module")
def harness(L):
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "log_read.mk", "liblog_read_harness.so"], check=True)
    lib = ctypes.CDLL(os.path.join(NATIVE, "liblog_read_harness.so"))
    vp, u64, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t
    lib.shim_log_read_device.restype = ctypes.c_int
    lib.shim_log_read_device.argtypes = [vp, sz, ctypes.c_int, u64, vp, vp, sz, vp]
    return lib


@pytest.mark.gpu
def test_reference_traces_through_the_device_reader(harness, fixture_images, port):
    _need_gpu()
    import torch
    for c, bad in fixture_images:
        d = _device_copy(bad)
        torch.cuda.synchronize()
        cap = 64 * (len(bad) // 7 + 16) + 4096
        out = ctypes.create_string_buffer(cap)
        n = ctypes.c_size_t(0)
        rc = harness.shim_log_read_device(d.data_ptr() if len(bad) else None, len(bad), int(c["checksum"]),
                                          c["initial_offset"], None, out, cap, ctypes.byref(n))
        assert rc == 0, (c["name"], rc)
        trace = out.raw[:n.value].decode()
        if "trace" in c:
            assert trace == c["trace"], c["name"]
        else:
            assert (port.value(trace.encode()), trace.count("\n")) == (c["trace_crc"], c["trace_lines"]), c["name"]


@pytest.mark.gpu
def test_identity_on_the_reference_images(L, fixture_images):
    _need_gpu()
    nrec = nrep = 0
    for c, bad in fixture_images:
        want = check_identity(L, bad, c["initial_offset"], int(c["checksum"]), c["name"])
        nrec += want[0][0]
        nrep += want[0][1]
    assert nrec > 1000 and nrep > 100, (nrec, nrep)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 1, 3, 15])
def test_edge_images(L, shift):
    _need_gpu()
    for name, img, initial_offset, checksum in lrc.edge_cases():
        check_identity(L, img, initial_offset, checksum, name, shift)


@pytest.mark.gpu
def test_header_fuzz(L):
    _need_gpu()
    nrec = nrep = 0
    for seed in range(200):
        img = fuzz_image(seed)
        for initial_offset in (0, 1 + 37 * seed):
            want = check_identity(L, img, initial_offset, 1, ("fuzz", seed, initial_offset), seed % 16)
            nrec += want[0][0]
            nrep += want[0][1]
    assert nrec > 500 and nrep > 1000, (nrec, nrep)  # (most fuzz fragments are orphans: reports, few records)


@pytest.mark.gpu
def test_scan_seams(L):
    _need_gpu()
    count = 0
    for name, img in seam_images():
        want = check_identity(L, img, 0, 1, name, 1)
        count += 1
        if name == "dense":
            import numpy as np
            assert int(np.frombuffer(want[1], dtype="<u4").reshape(-1, 8)[:, 6].max()) > 10000  # fragments of one record
    assert count == 1 + 3 * len(lrc.seam_positions())


@pytest.mark.gpu
@pytest.mark.parametrize("pre", [1, 2, 3])
def test_gather_edges(L, pre):
    _need_gpu()
    img = lrc.gather_image(pre)
    for payload_shift in (0, 1, 5):
        want = check_identity(L, img, 0, 1, ("gather", pre), pre, payload_shift=payload_shift)
    assert want[0][0] >= 3 * 9 and want[0][2] > 4 * 32761


@pytest.mark.gpu
def test_stream_query_and_capacity(L):
    _need_gpu()
    import torch
    img = lrc.gather_image(2)
    want = lrc.host_read(L, img)
    nr, nq, nb = want[0]
    d = _device_copy(img, 3)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        stream.synchronize()
        got = lrc.dev_read(L, d, len(img), 0, 1, stream.cuda_stream, want[0])
        assert got == want
        tot = L.LogReadTotals()
        rc = L.lib.nvl_log_read_dev(d.data_ptr(), len(img), 0, 1, None, 0, None, 0, None, 0, ctypes.byref(tot), 0,
                                    stream.cuda_stream)
        assert rc == 0 and (tot.n_records, tot.n_reports, tot.payload_bytes) == (nr, nq, nb)
        bad = dict((n, i) for n, i, _o, _c in lrc.edge_cases())["lone_middle"]
        (br, bq, bb) = lrc.host_read(L, bad)[0]
        db = _device_copy(bad)
        stream.synchronize()
        assert br and bq and bb
        rec, rep = (L.LogRecord * br)(), (L.LogReport * bq)()
        pay = torch.empty(bb, dtype=torch.uint8, device="cuda")
        for short in range(3):
            caps = [bb, br, bq]
            caps[short] -= 1
            tot = L.LogReadTotals()
            rc = L.lib.nvl_log_read_dev(db.data_ptr(), len(bad), 0, 1, pay.data_ptr(), caps[0], rec, caps[1], rep,
                                        caps[2], ctypes.byref(tot), 0, stream.cuda_stream)
            assert rc == L.ENOSPC and (tot.n_records, tot.n_reports, tot.payload_bytes) == (br, bq, bb), short


@pytest.mark.gpu
def test_python_view():
    _need_gpu()
    import torch
    from nvlevelz_amd import framing
    cases = dict((n, (i, o)) for n, i, o, _c in lrc.edge_cases())
    for name in ("three_blocks", "three_blocks_from_28", "unknown_inside", "checksum_inside_fragment"):
        img, io = cases[name]
        want = framing.log_read(img, initial_offset=io, host=True)
        got = framing.log_read_dev(torch.frombuffer(bytearray(img), dtype=torch.uint8).cuda(), initial_offset=io)
        assert got.reports == want.reports and got.records.tobytes() == want.records.tobytes(), name
        assert got.payload.is_cuda and got.payload.cpu().numpy().tobytes() == want.payload, name
        for k in range(len(want.records)):
            assert got.record_bytes(k) == want.record_bytes(k), (name, k)


@pytest.mark.gpu
def test_windows_of_1_and_3_blocks():
    """NVL_LOG_DEV_WINDOW_BLOCKS is read once per process: one fresh child per
    value, one after the other."""
    _need_gpu()
    for wb in ("1", "3"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, NVL_LOG_DEV_WINDOW_BLOCKS=wb))
        assert r.returncode == 0, (wb, r.stdout[-2000:], r.stderr[-4000:])
        assert "windows ok" in r.stdout, (wb, r.stdout)


if __name__ == "__main__":
    seen = run_edge_seam_gather(_lib())
    assert seen[0] > 100 and seen[1] > 1000 and seen[2] > 10000, seen
    print("windows ok", os.environ.get("NVL_LOG_DEV_WINDOW_BLOCKS"), seen)
