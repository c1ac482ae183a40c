"""The log record reader (include/nvl_framing.h: nvl_log_read, nvl_log_read_dev;
rules nvlevelz_amd/csrc/crc32c_log_read_core.h), CPU side: nvl_log_read with
the host CRC must reproduce the REFERENCE's log::Reader traces --

* tests/golden/log_cases.json: the 346 scenarios of tests/test_framing.py;
* tests/golden/log_read_cases.json: record-level edge images
  (tests/log_read_cases.py:edge_cases), their traces recorded from the
  reference by tools/gen_log_read_golden.py; compared live as well where
  oracle/_ref/libref_framing.so is built --

plus the entry points' argument and capacity rules, the no-GPU behaviour of
the device entry, the kernels' resource usage and a host-only ASan/UBSan run
of the rules.  The GPU side is tests/test_log_read_dev.py.
"""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import log_read_cases as lrc
from conftest import ROOT, load_golden
from test_log_scan_dev import HIPCC, HOST, fixture_images, gpu_present, shim  # noqa: F401  (fixtures)

NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.fixture(scope="module")
def L():
    from nvlevelz_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def edge(port):
    """[(golden case, image)] of the record-level edge cases."""
    gold = {c["name"]: c for c in load_golden("log_read_cases")["cases"]}
    out = []
    for name, img, initial_offset, checksum in lrc.edge_cases():
        c = gold[name]
        assert (c["initial_offset"], c["checksum"], c["image_len"], c["image_crc"]) == \
            (initial_offset, bool(checksum), len(img), port.value(img)), name
        out.append((c, img))
    assert len(out) == len(gold)
    return out


def test_reference_traces(L, fixture_images, port):
    reasons = set()
    offsets = 0
    for c, bad in fixture_images:
        got = lrc.render(lrc.host_read(L, bad, c["initial_offset"], int(c["checksum"])), port.value)
        offsets += c["initial_offset"] > 0
        if "trace" in c:
            assert got == c["trace"], c["name"]
            reasons.update(re.findall(r"Corruption: ([a-z ]+(?:\(\d\))?)", got))
        else:
            assert (port.value(got.encode()), got.count("\n")) == (c["trace_crc"], c["trace_lines"]), c["name"]
    assert len(fixture_images) == 346 and offsets >= 100
    assert len(reasons) == 8, reasons  # every reason string occurs in the goldens


def test_edge_traces(L, edge, port):
    seen = ""
    for c, img in edge:
        got = lrc.render(lrc.host_read(L, img, c["initial_offset"], int(c["checksum"])), port.value)
        assert got == c["trace"], c["name"]
        seen += got
    for text in lrc.REASONS[1:8] + ("unknown record type 7", "unknown record type 0", "Corruption: error in middle of record"):
        assert text in seen, text
    assert "C 0 Corruption: error in middle of record" in seen  # after a zero-length FIRST


def test_edge_traces_vs_reference_live(L, edge, port):
    import oracle
    if not oracle.ref_framing_available():
        pytest.skip("oracle/_ref/libref_framing.so not built")
    rf = oracle.ref_framing()
    for c, img in edge:
        want = rf.log_read(img, c["checksum"], c["initial_offset"])
        assert want == c["trace"], c["name"]
        assert lrc.render(lrc.host_read(L, img, c["initial_offset"], int(c["checksum"])), port.value) == want, c["name"]


def test_records_are_packed(L, edge):
    for c, img in edge:
        (nr, _nq, nb), rec, _rep, _p = lrc.host_read(L, img, c["initial_offset"], int(c["checksum"]))
        r = np.frombuffer(rec, dtype="<u8").reshape(-1, 4)
        at = 0
        for k in range(nr):
            assert r[k, 1] == at, (c["name"], k)
            at += int(r[k, 2])
        assert at == nb, c["name"]


def _call(L, img, payload, pcap, rec, rcap, rep, qcap, tot, flags=HOST, dev=False, initial_offset=0):
    if dev:
        return L.lib.nvl_log_read_dev(img, len(img), initial_offset, 1, payload, pcap, rec, rcap, rep, qcap, tot, flags,
                                      None)
    return L.lib.nvl_log_read(img, len(img), initial_offset, 1, payload, pcap, rec, rcap, rep, qcap, tot, flags)


def test_capacities_and_arguments(L):
    img = dict((n, i) for n, i, _o, _c in lrc.edge_cases())["lone_middle"]  # two records and a report
    want = lrc.host_read(L, img)
    (nr, nq, nb) = want[0]
    assert nr >= 1 and nq >= 1 and nb >= 1
    tot = L.LogReadTotals()
    rec, rep = (L.LogRecord * (nr + 1))(), (L.LogReport * (nq + 1))()
    payload = ctypes.create_string_buffer(nb + 1)
    # the totals-only query
    assert _call(L, img, None, 0, None, 0, None, 0, ctypes.byref(tot)) == 0
    assert (tot.n_records, tot.n_reports, tot.payload_bytes) == (nr, nq, nb)
    # each cap one short: ENOSPC with exact totals
    for short in range(3):
        caps = [nb, nr, nq]
        caps[short] -= 1
        tot = L.LogReadTotals()
        assert _call(L, img, payload, caps[0], rec, caps[1], rep, caps[2], ctypes.byref(tot)) == L.ENOSPC, short
        assert (tot.n_records, tot.n_reports, tot.payload_bytes) == (nr, nq, nb), short
    # the caps that always suffice
    n = len(img)
    rec2, rep2 = (L.LogRecord * (n // 7 + 1))(), (L.LogReport * (n // 7 + n // 32768 + 2))()
    pay2 = ctypes.create_string_buffer(n)
    assert _call(L, img, pay2, n, rec2, n // 7 + 1, rep2, n // 7 + n // 32768 + 2, ctypes.byref(tot)) == 0
    assert lrc._result(tot, rec2, rep2, pay2.raw[:nb]) == want
    # argument errors, checked before any HIP call: the same for both entries with or without a GPU
    for dev in (False, True):
        flags = 0 if dev else HOST
        assert _call(L, img, payload, nb, rec, nr, rep, nq, None, flags, dev) == L.EINVAL  # totals == NULL
        tot = L.LogReadTotals(7, 7, 7)
        if dev:  # data == NULL with a length
            rc = L.lib.nvl_log_read_dev(None, 15, 0, 1, payload, nb, rec, nr, rep, nq, ctypes.byref(tot), 0, None)
        else:
            rc = L.lib.nvl_log_read(None, 15, 0, 1, payload, nb, rec, nr, rep, nq, ctypes.byref(tot), HOST)
        assert rc == L.EINVAL
        assert (tot.n_records, tot.n_reports, tot.payload_bytes) == (0, 0, 0)
        assert _call(L, img, payload, nb, rec, nr, rep, nq, ctypes.byref(tot), 0x2000, dev) == L.EINVAL  # unknown flag
        # a skip to or past the end (from a block trailer too): nothing to read, no device needed
        for io in (lrc.BLK - 3, lrc.BLK, 5 * lrc.BLK + 9):
            tot = L.LogReadTotals(7, 7, 7)
            assert _call(L, img, payload, nb, rec, nr, rep, nq, ctypes.byref(tot), flags, dev, io) == 0
            assert (tot.n_records, tot.n_reports, tot.payload_bytes) == (0, 0, 0)
    assert _call(L, img, payload, nb, rec, nr, rep, nq, ctypes.byref(tot), lrc.PAYLOAD_HOST) == L.EINVAL  # dev's flag
    assert _call(L, img, payload, nb, rec, nr, rep, nq, ctypes.byref(tot), HOST | 0x400) == L.EINVAL  # both engines


def test_python_views(port):
    from nvlevelz_amd import framing
    cases = dict((n, (i, o, c)) for n, i, o, c in lrc.edge_cases())
    img, io, ck = cases["unknown_inside"]
    got = framing.log_read(img, host=True)
    assert got.reports == [(4 + 6 + 5, "unknown record type 7"), (2, "missing start of fragmented record(2)")]
    assert len(got.records) == 0 and got.payload == b""
    img, io, ck = cases["three_blocks"]
    got = framing.log_read(img, host=True)
    assert [int(x) for x in got.records["length"]] == [20, 3 * 32768 - 21 - 27 + 100, 50, 0]
    assert [int(x) for x in got.records["fragments"]] == [1, 4, 1, 1]
    assert got.record_bytes(0) == img[7:27] and got.record_bytes(2) == img[3 * 32768 + 107 + 7:3 * 32768 + 107 + 57]
    assert got.record_bytes(1)[-100:] == img[3 * 32768 + 7:3 * 32768 + 107]
    assert framing.log_read(img, initial_offset=28, host=True).records["offset"].tolist() == [3 * 32768 + 107, 3 * 32768 + 164]
    with pytest.raises(TypeError):
        framing.log_read_dev(bytes(15))
    with pytest.raises(TypeError):
        framing.log_read_dev(np.zeros(15, dtype=np.uint8))


@pytest.mark.skipif(gpu_present(), reason="checks the no-GPU behaviour")
def test_device_entry_fails_loudly_without_gpu(L):
    img = dict((n, i) for n, i, _o, _c in lrc.edge_cases())["lone_middle"]
    rec, rep = (L.LogRecord * 4)(), (L.LogReport * 4)()
    payload = ctypes.create_string_buffer(64)
    for buf in (rec, rep, payload):
        ctypes.memset(buf, 0xA5, ctypes.sizeof(buf))
    tot = L.LogReadTotals(7, 7, 7)
    for flags in (0, lrc.PAYLOAD_HOST):
        rc = L.lib.nvl_log_read_dev(img, len(img), 0, 1, payload, 64, rec, 4, rep, 4, ctypes.byref(tot), flags, None)
        assert rc in (L.ENODEV, L.EHIP)
        assert (tot.n_records, tot.n_reports, tot.payload_bytes) == (0, 0, 0)
        for buf in (rec, rep, payload):
            assert bytes(buf) == b"\xA5" * ctypes.sizeof(buf)  # nothing written


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("ru") / "crc32c_log_read.o"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "--offload-arch=gfx950",
                        "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
                        os.path.join(ROOT, "nvlevelz_amd", "csrc", "crc32c_log_read.hip"), "-o", str(out),
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
    names = ("crc32c_log_read_classify", "crc32c_log_read_reduce", "crc32c_log_read_tiles", "crc32c_log_read_apply",
             "crc32c_log_read_emit", "crc32c_log_read_gather")
    for name in names:
        hits = [k for k in usage if name in k]
        assert hits, (name, sorted(usage))
        for k in hits:
            u = usage[k]
            assert u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (k, u)
            assert u.get("ScratchSize", 0) <= 32, (k, u)
    assert len([k for k in usage if "crc32c_log_read_tiles" in k]) == 2  # one per scan


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_rules_under_asan(edge, tmp_path):
    """The rules header and nvl_log_read as a stand-alone host program under
    ASan/UBSan, inputs and outputs in exact-size heap blocks."""
    subprocess.run(["make", "-s", "-C", NATIVE, "-f", "log_read.mk", "log_read_asan"], check=True, timeout=300)
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for c, img in edge:
            f.write(struct.pack("<QQQ", len(img), c["initial_offset"], int(c["checksum"])) + img)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(NATIVE, "log_read_asan"), str(path)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    traces = r.stdout.split("=\n")
    assert traces[-1] == "" and len(traces) == len(edge) + 1
    for (c, _img), got in zip(edge, traces):
        assert got == c["trace"], c["name"]
