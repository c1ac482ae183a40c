"""The device-resident log scan (include/nvl_framing.h: nvl_log_scan_dev,
nvl_log_scan_staged; kernels nvlevelz_amd/csrc/crc32c_log_dev.hip): the record
headers are parsed, the CRCs checked and the events laid out on the GPU.

Parity anchors:
* tests/golden/log_cases.json -- the REFERENCE's own log::Reader traces
  (see tests/test_framing.py): every case through shims::LogReader with
  NVL_LOG_DEVICE_PARSE, whole image and streamed in windows of 1 and 3 blocks;
* nvl_log_scan(..., NVL_FRAMING_HOST): both device entry points must return
  exactly its events (every field, `reserved` included) on the fixtures'
  images, on synthetic edge images, on a seeded header fuzz, and with the
  window size forced to 1 and 3 blocks (NVL_LOG_DEV_WINDOW_BLOCKS, one child
  process each).  The host scan and the kernels run the same block rules
  (nvlevelz_amd/csrc/crc32c_log_core.h), so this comparison alone would pass
  a rule bug shared by both; the host side is anchored without a GPU: to the
  reference's traces by tests/test_framing.py, and on the edge and fuzz
  images of this module to the events recorded before the rules were shared
  (tests/test_log_scan_golden.py, tests/golden/log_scan_events.json).

Run as a script (the window children): `python tests/test_log_scan_dev.py`
checks the edge images and 20 fuzz seeds under the environment's window size.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HOST = 0x100
DEVICE_PARSE = 0x800
BLK = 32768
HIPCC = "/opt/rocm/bin/hipcc"
KINDS = ("RECORD", "BAD_LENGTH", "CHECKSUM", "ZERO", "EOF")


def gpu_present() -> bool:
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _lib():
    from nvlevelz_amd import _lib as L
    return L


# ------------------------------------------------------------ image builders --

class Log:
    """A log image under construction: headers with a zero CRC, sealed by the
    host writer (nvl_log_seal, NVL_FRAMING_HOST), then optional byte edits."""

    def __init__(self, rng):
        self.rng = rng
        self.buf = bytearray()
        self.hdrs = []

    def record(self, n, rtype=1, seal=True):
        if seal:
            self.hdrs.append(len(self.buf))
        self.buf += bytes(4) + bytes([n & 0xFF, n >> 8, rtype]) + self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        return self

    def raw(self, b):
        self.buf += b
        return self

    def garbage(self, n, nonzero=False):
        self.buf += self.rng.integers(1 if nonzero else 0, 256, n, dtype=np.uint8).tobytes()
        return self

    def fill_block(self, end, sizes=(0, 1, 5, 100, 1000, 3000)):
        """Records until the image is exactly `end` bytes long."""
        while len(self.buf) < end:
            room = end - len(self.buf) - 7
            assert room >= 0
            n = int(self.rng.choice(sizes))
            if n > room or 0 < room - n < 7:  # never leave a gap of 1..6 bytes
                n = room
            self.record(n, int(self.rng.integers(1, 5)))
        return self

    def sealed(self):
        L = _lib()
        img = bytearray(self.buf)
        if self.hdrs:
            off = np.array(self.hdrs, dtype=np.uint64)
            buf = (ctypes.c_char * len(img)).from_buffer(img)
            assert L.lib.nvl_log_seal(buf, len(img), off.ctypes.data, len(off), HOST) == 0
            del buf
        return img


def edge_images():
    """(name, bytes) of the synthetic edge images."""
    rng = np.random.default_rng(20240607)
    out = []

    def add(name, img):
        out.append((name, bytes(img)))

    for n in (0, 1, 6, 7, 8):
        add(f"random_{n}", Log(rng).garbage(n).buf)
    add("valid_7", Log(rng).record(0).sealed())
    add("valid_8", Log(rng).record(1).sealed())
    add("exact_1_block", Log(rng).fill_block(BLK).sealed())
    add("exact_2_blocks", Log(rng).fill_block(BLK).fill_block(2 * BLK).sealed())
    lg = Log(rng)
    for _ in range(4681):
        lg.record(0)
    add("4681_records_trailer", lg.raw(b"\x07").record(20).sealed())
    add("record_ends_block_then_more", Log(rng).fill_block(BLK).record(300).record(0).sealed())
    for t in range(1, 7):
        add(f"trailer_{t}", Log(rng).fill_block(BLK - t).garbage(t, nonzero=True).record(40).sealed())
    lg = Log(rng).fill_block(BLK)
    lg.record(50).raw(bytes(4) + (60000).to_bytes(2, "little") + b"\x01").fill_block(2 * BLK).fill_block(3 * BLK).record(9)
    add("bad_length_middle", lg.sealed())
    lg = Log(rng).fill_block(BLK).record(70).raw(bytes(7)).garbage(BLK - 84).fill_block(3 * BLK).record(9)
    add("zero_middle", lg.sealed())
    add("zero_last", Log(rng).fill_block(BLK).record(10).raw(bytes(7)).garbage(30).sealed())
    add("truncated_header_last", Log(rng).fill_block(BLK).record(10).garbage(3, nonzero=True).sealed())
    lg = Log(rng).fill_block(BLK).record(10)
    add("truncated_payload_last", lg.raw(bytes(4) + (100).to_bytes(2, "little") + b"\x01").garbage(50).sealed())
    for where in ("first", "last"):
        lg = Log(rng).fill_block(BLK)
        first = len(lg.buf)
        lg.fill_block(2 * BLK)
        last = max(h for h in lg.hdrs if h < 2 * BLK)
        img = lg.fill_block(3 * BLK).record(33).sealed()
        img[(first if where == "first" else last) + 1] ^= 0x10
        add(f"mismatch_{where}_of_block", img)
    img = Log(rng).fill_block(BLK).record(10).record(200).record(5).sealed()
    img[BLK + 17 + 2] ^= 0x01
    add("mismatch_in_short_last_block", img)
    img = Log(rng).fill_block(BLK).record(10).sealed()
    img[BLK + 8] ^= 0x80  # payload byte of the only record of the last block
    add("mismatch_only_record_of_last_block", img)
    add("random_3_blocks", Log(rng).garbage(3 * BLK).buf)
    return out


def fuzz_image(seed):
    """0-3 whole blocks and a tail, each walked writing sealed records of
    biased lengths with injected header faults."""
    rng = np.random.default_rng(77000 + seed)
    tail = int(rng.choice([0, 1, 6, 7, 8, 100, 5000, 32767]))
    sizes = [BLK] * int(rng.integers(0, 4)) + [tail]
    lg = Log(rng)
    flips = []
    for m in sizes:
        b0 = len(lg.buf)
        lg.garbage(m)
        pos = 0
        while m - pos >= 7:
            if rng.random() < 0.02:
                break  # stop and leave garbage
            room = m - pos - 7
            pick = int(rng.integers(0, 8))
            n = (0, 0, 1, 5, 100, 1000, room, int(rng.integers(0, room + 1)))[pick]
            n = min(n, room)
            h = b0 + pos
            fault = rng.random()
            if fault < 0.04:  # a length field that runs past the block
                over = min(65535, room + 1 + int(rng.integers(0, 300)))
                lg.buf[h + 4:h + 7] = over.to_bytes(2, "little") + b"\x01"
                break
            if fault < 0.08:  # a zeroed header
                lg.buf[h:h + 7] = bytes(7)
                break
            lg.buf[h:h + 7] = bytes(4) + n.to_bytes(2, "little") + bytes([int(rng.integers(1, 5))])
            lg.hdrs.append(h)
            if fault < 0.13:
                flips.append((h + int(rng.integers(0, 4)), 1 << int(rng.integers(0, 8))))
            pos += 7 + n
    img = lg.sealed()
    for at, bit in flips:
        img[at] ^= bit
    return bytes(img)


# ---------------------------------------------------------- the three scans --

def _events(ev, n):
    return bytes(ev)[:n * 32]


def host_scan(L, img, start, checksum):
    """nvl_log_scan with the host CRC: (count, the events' bytes)."""
    n = ctypes.c_size_t(0)
    assert L.lib.nvl_log_scan(img, len(img), start, checksum, None, 0, ctypes.byref(n), HOST) == 0
    ev = (L.LogEvent * max(n.value, 1))()
    assert L.lib.nvl_log_scan(img, len(img), start, checksum, ev, n.value, ctypes.byref(n), HOST) == 0
    return n.value, _events(ev, n.value)


def _describe(L, raw):
    a = np.frombuffer(raw, dtype=np.dtype([("offset", "<u8"), ("block_end", "<u8"), ("length", "<u4"), ("type", "<u4"),
                                           ("kind", "<u4"), ("reserved", "<u4")]))
    return [tuple(int(x) for x in e) for e in a[:12]], len(a)


def check_identity(L, img, dimg, start, checksum, stream, what):
    """Both new entry points return exactly the host scan's events; returns
    the kinds seen.  dimg: a device tensor holding img."""
    want_n, want = host_scan(L, img, start, checksum)
    cap = want_n + 2
    for path in ("dev", "staged"):
        ev = (L.LogEvent * cap)()
        n = ctypes.c_size_t(0)
        if path == "dev":
            rc = L.lib.nvl_log_scan_dev(dimg.data_ptr() if len(img) else None, len(img), start, checksum, ev, cap,
                                        ctypes.byref(n), stream)
        else:
            rc = L.lib.nvl_log_scan_staged(img, len(img), start, checksum, ev, cap, ctypes.byref(n))
        assert rc == 0, (what, path, rc)
        got = _events(ev, min(n.value, cap))
        assert (n.value, got) == (want_n, want), (what, path, start, checksum, n.value, want_n, _describe(L, got),
                                                  _describe(L, want))
    kinds = np.frombuffer(want, dtype="<u4").reshape(-1, 8)[:, 6]
    return np.bincount(kinds, minlength=5)


def _device_copy(img, shift=0):
    """img in device memory, starting `shift` bytes into its allocation."""
    import torch
    t = torch.empty(len(img) + shift + 16, dtype=torch.uint8, device="cuda")
    if len(img):
        t[shift:shift + len(img)] = torch.frombuffer(bytearray(img), dtype=torch.uint8)
    return t[shift:shift + len(img)]


def run_edge_and_fuzz(L, seeds, shifts=(0, 1, 3, 15)):
    """The edge images (every allocation shift, a non-default stream) and the
    fuzz seeds through check_identity; returns the kind counts."""
    import torch
    stream = torch.cuda.Stream()
    seen = np.zeros(5, dtype=np.int64)
    with torch.cuda.stream(stream):
        for name, img in edge_images():
            for shift in shifts:
                d = _device_copy(img, shift)
                stream.synchronize()
                for checksum in (1, 0):
                    seen += check_identity(L, img, d, 0, checksum, stream.cuda_stream, (name, shift))
        for seed in seeds:
            img = fuzz_image(seed)
            d = _device_copy(img, seed % 16)
            stream.synchronize()
            for start in (0, 3 * BLK):
                for checksum in (1, 0):
                    k = check_identity(L, img, d, start, checksum, stream.cuda_stream, ("fuzz", seed))
                    if start == 0 and checksum:
                        seen += k
    return seen


# ----------------------------------------------------------------- fixtures --

@pytest.fixture(scope="module")
def L():
    return _lib()


@pytest.fixture(scope="module")
def shim(L):
    native = os.path.join(ROOT, "tests", "native")
    path = os.path.join(native, "libshim_harness.so")
    # (make rebuilds it only when the shim header or the engine is newer: the reader under test is header-only)
    subprocess.run(["make", "-s", "-C", native, "libshim_harness.so"], check=True)
    lib = ctypes.CDLL(path)
    vp, u64, sz, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_uint32
    lib.shim_log_write.restype = ctypes.c_int
    lib.shim_log_write.argtypes = [vp, vp, sz, u64, u32, vp, sz, vp]
    lib.shim_log_read.restype = ctypes.c_int
    lib.shim_log_read.argtypes = [vp, sz, ctypes.c_int, u64, u32, vp, sz, vp]
    lib.shim_log_read_stream.restype = ctypes.c_int
    lib.shim_log_read_stream.argtypes = [vp, sz, ctypes.c_int, u64, u32, sz, u64, vp, sz, vp, vp]
    return lib


def _shim_read(shim, image, checksum, initial_offset, flags, window_blocks=None):
    """(rc, trace) of shims::LogReader over image (streamed when window_blocks)."""
    cap = 64 * (len(image) // 7 + 16) + 4096
    out = ctypes.create_string_buffer(cap)
    n = ctypes.c_size_t(0)
    if window_blocks is None:
        rc = shim.shim_log_read(image or b"\0", len(image), int(checksum), initial_offset, flags, out, cap,
                                ctypes.byref(n))
    else:
        reads = ctypes.c_size_t(0)
        rc = shim.shim_log_read_stream(image or b"\0", len(image), int(checksum), initial_offset, flags,
                                       window_blocks, (1 << 64) - 1, out, cap, ctypes.byref(n), ctypes.byref(reads))
    return rc, out.raw[:n.value].decode()


@pytest.fixture(scope="module")
def fixture_images(shim, port):
    """The 346 reference cases: (case, the image the reference read), written
    with the host writer and mutated as the fixture says."""
    import framing_cases as fc
    from conftest import load_golden
    cases = load_golden("log_cases")["cases"]
    assert len(cases) >= 300

    def w(payloads, dest_length):
        blob = b"".join(payloads) or b"\0"
        lens = np.array([len(p) for p in payloads] or [0], dtype=np.uint64)
        total = sum(len(p) for p in payloads)
        cap = total + 7 * (total // 8 + len(payloads) + 2) + 64
        out = ctypes.create_string_buffer(cap)
        n = ctypes.c_size_t(0)
        assert shim.shim_log_write(blob, lens.ctypes.data, len(payloads), dest_length, HOST, out, cap,
                                   ctypes.byref(n)) == 0
        return out.raw[:n.value]

    out = []
    for c in cases:
        bad = fc.mutate(port, fc.write_image(port, c, w), c["mutations"])
        assert (len(bad), port.value(bad)) == (c["read_len"], c["read_crc"]), c["name"]
        out.append((c, bad))
    return out


# ---------------------------------------------------------------------- CPU --

def test_argument_errors(L):
    """Checked before any HIP call: the same on a machine without a GPU."""
    ev = (L.LogEvent * 4)()
    n = ctypes.c_size_t(7)
    img = bytes(15)
    lib = L.lib
    assert lib.nvl_log_scan_dev(img, 15, 0, 1, ev, 4, None, None) == L.EINVAL  # n_events == NULL
    assert lib.nvl_log_scan_staged(img, 15, 0, 1, ev, 4, None) == L.EINVAL
    assert lib.nvl_log_scan_dev(img, 15, 5, 1, ev, 4, ctypes.byref(n), None) == L.EINVAL  # start % 32768
    assert lib.nvl_log_scan_staged(img, 15, 32767, 1, ev, 4, ctypes.byref(n)) == L.EINVAL
    assert lib.nvl_log_scan_dev(None, 15, 0, 1, ev, 4, ctypes.byref(n), None) == L.EINVAL  # NULL with len
    assert lib.nvl_log_scan_staged(None, 15, 0, 1, ev, 4, ctypes.byref(n)) == L.EINVAL
    assert n.value == 0 and bytes(ev) == bytes(4 * 32)


def test_python_view_rejects_host_bytes():
    from nvlevelz_amd import framing
    with pytest.raises(TypeError):
        framing.log_scan_dev(bytes(15))
    with pytest.raises(TypeError):
        framing.log_scan_dev(np.zeros(15, dtype=np.uint8))


@pytest.mark.skipif(gpu_present(), reason="checks the no-GPU behaviour")
def test_fails_loudly_without_gpu(L, shim):
    log = b"\x01\x02\x03\x04\x01\x00\x01x" + bytes(7)
    assert len(log) == 15
    ev = (L.LogEvent * 4)()
    ctypes.memset(ev, 0xA5, ctypes.sizeof(ev))
    n = ctypes.c_size_t(0)
    assert L.lib.nvl_log_scan_staged(log, 15, 0, 1, ev, 4, ctypes.byref(n)) in (L.ENODEV, L.EHIP)
    assert bytes(ev) == b"\xA5" * ctypes.sizeof(ev) and n.value == 0  # nothing written
    rc, trace = _shim_read(shim, log, 1, 0, DEVICE_PARSE)
    assert rc in (L.ENODEV, L.EHIP) and trace == ""  # non-OK status, no records
    rc, trace = _shim_read(shim, log, 1, 0, DEVICE_PARSE, window_blocks=1)
    assert rc in (L.ENODEV, L.EHIP) and trace == ""


def test_device_parse_with_host_engine_is_an_argument_error(L, shim):
    log = b"\x01\x02\x03\x04\x01\x00\x01x" + bytes(7)
    rc, trace = _shim_read(shim, log, 1, 0, HOST | DEVICE_PARSE)
    assert rc == L.EINVAL and trace == ""
    rc, trace = _shim_read(shim, log, 1, 0, HOST | DEVICE_PARSE, window_blocks=3)
    assert rc == L.EINVAL and trace == ""
    from nvlevelz_amd import framing
    with pytest.raises(ValueError):
        framing.log_scan(log, host=True, device_parse=True)


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("ru") / "crc32c_log_dev.o"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "--offload-arch=gfx950",
                        "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
                        os.path.join(ROOT, "nvlevelz_amd", "csrc", "crc32c_log_dev.hip"), "-o", str(out),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            kernels[cur][m.group(1).strip()] = int(m.group(2))
    return kernels


def test_kernel_resources(usage):
    """No spills, and a staged block small enough that four parse waves share
    a CU's 160 KiB of LDS (the serial header walk of one hides behind the
    others' loads)."""
    names = ("crc32c_log_parse", "crc32c_log_scan", "crc32c_log_expand", "crc32c_log_verdict", "crc32c_log_emit")
    for name in names:
        hits = [k for k in usage if name in k]
        assert hits, (name, sorted(usage))
        for k in hits:
            u = usage[k]
            assert u.get("VGPRs Spill", 0) == 0, (k, u)
            assert u.get("ScratchSize", 0) <= 32, (k, u)
    parse = [usage[k] for k in usage if "crc32c_log_parse" in k][0]
    assert 32768 <= parse["LDS Size"] <= 40 * 1024, parse
    assert 4 * parse["LDS Size"] <= 160 * 1024


# ---------------------------------------------------------------------- GPU --

def _need_gpu():
    if not gpu_present():
        pytest.skip("no GPU")


def _block_start(initial_offset):
    """SkipToInitialBlock as LogReader::Scan does it (log_reader.cc:36-60)."""
    in_block = initial_offset % BLK
    start = initial_offset - in_block
    return start + BLK if in_block > BLK - 6 else start


@pytest.mark.gpu
def test_reference_traces_through_the_shim(shim, fixture_images, port):
    _need_gpu()
    for c, bad in fixture_images:
        for wb in (None, 1, 3):
            rc, trace = _shim_read(shim, bad, c["checksum"], c["initial_offset"], DEVICE_PARSE, wb)
            assert rc == 0, (c["name"], wb, rc)
            if "trace" in c:
                assert trace == c["trace"], (c["name"], wb)
            else:
                assert (port.value(trace.encode()), trace.count("\n")) == (c["trace_crc"], c["trace_lines"]), \
                    (c["name"], wb)


@pytest.mark.gpu
def test_event_identity_on_the_reference_images(L, fixture_images):
    _need_gpu()
    import torch
    seen = np.zeros(5, dtype=np.int64)
    for c, bad in fixture_images:
        d = _device_copy(bad)
        torch.cuda.synchronize()
        starts = {0, _block_start(c["initial_offset"])}
        for start in sorted(s for s in starts if s == 0 or s < len(bad)):
            part = bad[start:]
            dp = d[start:]
            for checksum in (1, 0):
                seen += check_identity(L, part, dp, start, checksum, None, c["name"])
    assert seen[0] > 0 and seen[4] > 0, seen


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 1, 3, 15])
def test_edge_images(L, shift):
    _need_gpu()
    seen = run_edge_and_fuzz(L, (), shifts=(shift,))
    assert all(seen > 0), dict(zip(KINDS, seen))  # the edge images reach every kind of event


@pytest.mark.gpu
def test_header_fuzz(L):
    _need_gpu()
    import torch
    seen = np.zeros(5, dtype=np.int64)
    total = 0
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for seed in range(200):
            img = fuzz_image(seed)
            total += len(img)
            d = _device_copy(img, seed % 16)
            stream.synchronize()
            for start in (0, 3 * BLK):
                for checksum in (1, 0):
                    k = check_identity(L, img, d, start, checksum, stream.cuda_stream, ("fuzz", seed))
                    if start == 0 and checksum:
                        seen += k
    print("fuzz: %d bytes, events %s" % (total, dict(zip(KINDS, seen))))
    assert all(seen > 0), dict(zip(KINDS, seen))  # every kind of event was exercised
    assert seen[4] == 200


@pytest.mark.gpu
def test_capacity(L):
    _need_gpu()
    import torch
    for name, img in edge_images():
        want_n, want = host_scan(L, img, 0, 1)
        d = _device_copy(img, 3)
        torch.cuda.synchronize()
        for path in ("dev", "staged"):
            def scan(ev, cap, n):
                if path == "dev":
                    return L.lib.nvl_log_scan_dev(d.data_ptr() if len(img) else None, len(img), 0, 1, ev, cap, n, None)
                return L.lib.nvl_log_scan_staged(img, len(img), 0, 1, ev, cap, n)
            n = ctypes.c_size_t(0)
            assert scan(None, 0, ctypes.byref(n)) == 0 and n.value == want_n, (name, path)  # the count only
            cap = want_n - 1
            ev = (L.LogEvent * (cap + 2))()
            ctypes.memset(ev, 0xA5, ctypes.sizeof(ev))
            assert scan(ev, cap, ctypes.byref(n)) == L.ENOSPC, (name, path)
            assert n.value == want_n, (name, path)
            raw = bytes(ev)
            assert raw[:cap * 32] == want[:cap * 32], (name, path)
            assert raw[cap * 32:] == b"\xA5" * 64, (name, path)  # nothing past cap


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


@pytest.mark.gpu
def test_python_view(port):
    """framing.log_scan_dev and log_scan(device_parse=True) against
    log_scan(host=True) on the image of tests/test_framing.py::test_python_view_log."""
    _need_gpu()
    import torch
    from nvlevelz_amd import framing
    img, hdrs = bytearray(), []
    for k, n in enumerate([10, 300, 0, 5000]):
        hdrs.append(len(img))
        img += bytes(4) + bytes([n & 0xFF, n >> 8, 1]) + port.fill(k, 0, n).tobytes()
    framing.log_seal(img, hdrs, host=True)
    bad = bytearray(img)
    bad[hdrs[1] + 9] ^= 1
    for image in (bytes(img), bytes(bad)):
        want = framing.log_scan(image, host=True)
        d = torch.frombuffer(bytearray(image), dtype=torch.uint8).cuda()
        assert framing.log_scan_dev(d) == want
        assert framing.log_scan_dev(d, checksum=False) == framing.log_scan(image, host=True, checksum=False)
        assert framing.log_scan(image, device_parse=True) == want
        assert framing.log_scan(np.frombuffer(image, dtype=np.uint8), device_parse=True, start=BLK) == \
            framing.log_scan(image, host=True, start=BLK)
    assert [e[0] for e in framing.log_scan_dev(torch.frombuffer(bad, dtype=torch.uint8).cuda())] == \
        ["record", "checksum mismatch", "eof"]


if __name__ == "__main__":
    seen = run_edge_and_fuzz(_lib(), range(20))
    assert all(seen > 0), seen
    print("windows ok", os.environ.get("NVL_LOG_DEV_WINDOW_BLOCKS"), dict(zip(KINDS, (int(x) for x in seen))))
