"""Latency of the call-site shims at the fork's real sizes, GPU against the
host CRC, one JSON line per (operation, size, engine):

  seal         nvl_sstable_seal_trailers over a table image (BatchingWritableFile's
               Close, table/table_builder.cc:185-187 deferred); host-resident image
  seal_tb      the reference's own TableBuilder (oracle/_ref/libref_table.so)
               writing a table through shims::BatchingWritableFile, sealed at
               Close -- the whole build, GPU seal against host seal
  verify       nvl_sstable_verify_table (Table::Open + ReadBlock of every block,
               table/format.cc:65-98), host-resident image
  verify_dev   nvl_sstable_verify_table_dev, the image already in HBM
  window64     nvl_sstable_verify_blocks over 64 data blocks (shims::TableReader's
               readahead window, db/version_set.cc:1308,1329)
  manifest10   nvl_log_seal of a 10-record MANIFEST batch (db/version_set.cc:896-909,
               db/log_writer.cc:84-109)
  log_scan     (--log-scan 64,1024 only) nvl_log_scan_dev on an HBM-resident sealed log,
               nvl_log_scan_staged and nvl_log_scan (GPU / host CRC) on the same image in
               registered host memory, with the calling thread's CPU seconds per GiB, and
               the parse path beside nvl_crc32c_read_probe (profiles/log_scan_dev.jsonl)
  log_read     (--log-read 64,1024 only) nvl_log_read_dev (payload in HBM, and NVL_LOG_PAYLOAD_HOST)
               on an HBM-resident log written as log::Writer fragments it, against nvl_log_scan_dev
               on the same image and against what a caller had to do before: the image copied to
               the host, then a shims::LogReader ReadRecord loop with the host CRC; the legs
               alternate round by round; plus the gather kernel's share beside a plain
               device-to-device copy of the payload bytes (profiles/log_read_dev.jsonl)
Sizes: tables of 256 KiB .. 128 MiB (max_file_size is 2 MiB, util/options.cc:24;
compaction outputs and L0 flushes, db/builder.cc:35-45, db/db_impl.cc:923).
Wall clock per call (synchronous entry points), median of R calls after 2 warm-ups.
    python tools/shim_latency.py [--reps 15] [--out gpurun_out/shim_latency.jsonl]
"""
import argparse, ctypes, json, os, sys, time
ROOT = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from nvlevelz_amd import _lib
import bench

L = _lib.lib
HOST = _lib.FRAMING_HOST
GPU = getattr(_lib, "FRAMING_GPU", 0)
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=None)
ap.add_argument("--sizes", default="0.25,2,8,32,128", help="table sizes in MiB")
ap.add_argument("--log-scan", default=None, metavar="MIB,...",
                help="run only the device log scan legs on sealed logs of these sizes (e.g. 64,1024)")
ap.add_argument("--log-read", default=None, metavar="MIB,...",
                help="run only the device log reader legs on written logs of these sizes (e.g. 64,1024)")
ap.add_argument("--rounds", type=int, default=5, help="--log-read: alternating rounds of all legs")
ap.add_argument("--log-shapes", default="100B,1KiB,32KiB", help="record shapes of the --log-scan legs")
a = ap.parse_args()
out = open(a.out, "w") if a.out else None


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def med(fn, reps):
    fn(); fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def table_handles(img_len, nblocks):
    stride = 4096 + 5
    return np.stack([np.arange(nblocks, dtype=np.uint64) * stride, np.full(nblocks, 4096, np.uint64)], 1)


import torch
torch.cuda.set_device(0)
rc0 = L.nvl_crc32c_init(0)
assert rc0 == 0, f"nvl_crc32c_init: {rc0}"
sptr = torch.cuda.current_stream().cuda_stream


def sealed_log(mib, payload, seed=11):
    """A sealed log image of mib MiB: every 32 KiB block holds records of
    `payload` bytes and one last record filling the block (a trailer of fewer
    than 7 bytes stays zero, db/log_writer.cc:45-57); random payloads, headers
    sealed by nvl_log_seal.  Returns the image (numpy) and its record count."""
    nblk = int(mib * 2**20) // 32768
    pos, p = [], 0
    while 32768 - p >= 7:
        n = payload if 32768 - p - 7 - payload >= 7 else 32768 - p - 7
        pos.append((p, n))
        p += 7 + n
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, nblk * 32768, dtype=np.uint8)
    blocks = img.reshape(nblk, 32768)
    blocks[:, p:] = 0
    for q, n in pos:
        blocks[:, q + 4] = n & 0xFF
        blocks[:, q + 5] = n >> 8
        blocks[:, q + 6] = 1 if n == payload else 4
    hdr = (np.arange(nblk, dtype=np.uint64)[:, None] * np.uint64(32768) +
           np.array([q for q, _ in pos], dtype=np.uint64)[None, :]).ravel()
    rc = L.nvl_log_seal(img.ctypes.data, img.size, hdr.ctypes.data, hdr.size, GPU)
    assert rc == 0, rc
    return img, hdr.size


def log_scan_legs(sizes, reps):
    """nvl_log_scan_dev / nvl_log_scan_staged against nvl_log_scan (unchanged
    by the device log scan: the parent commit's code) on the same sealed log:
      (a) dev      the image in HBM (HIP events around the call as well)
      (b) staged   from registered host memory
      (c) scan_gpu nvl_log_scan, NVL_FRAMING_GPU, the same registered image
      (d) scan_host nvl_log_scan, NVL_FRAMING_HOST
    with the calling thread's CPU seconds per GiB, plus the parse path alone
    (nvl_log_scan_dev, checksum = 0, count only: parse, scans, verdict) beside
    nvl_crc32c_read_probe over the same bytes."""
    for mib in sizes:
        for payload, shape in ((100, "100B"), (1024, "1KiB"), (32761, "32KiB")):
            if shape not in a.log_shapes.split(","):
                continue
            img, nrec = sealed_log(mib, payload)
            nbytes = img.size
            gib = nbytes / 2**30
            cap = nrec + nbytes // 32768 + 4
            ev = (_lib.LogEvent * cap)()
            n = ctypes.c_size_t(0)
            base = {"log_bytes": nbytes, "records": nrec, "shape": shape}
            assert L.nvl_crc32c_host_register(img.ctypes.data, nbytes) == 0
            dimg = torch.from_numpy(img).to("cuda")
            torch.cuda.synchronize()
            want = nrec + 1  # every record and the final EOF

            def timed(fn, reps):
                fn(); fn()
                wall, cpu = [], []
                for _ in range(reps):
                    c0, t0 = time.thread_time(), time.perf_counter()
                    fn()
                    wall.append(time.perf_counter() - t0)
                    cpu.append(time.thread_time() - c0)
                return float(np.median(wall)), float(np.min(wall)), float(np.median(cpu))

            def check(rc):
                assert rc == 0 and n.value == want, (rc, n.value, want)

            legs = (
                ("dev", lambda: check(L.nvl_log_scan_dev(dimg.data_ptr(), nbytes, 0, 1, ev, cap, ctypes.byref(n), sptr))),
                ("staged", lambda: check(L.nvl_log_scan_staged(img.ctypes.data, nbytes, 0, 1, ev, cap, ctypes.byref(n)))),
                ("scan_gpu", lambda: check(L.nvl_log_scan(img.ctypes.data, nbytes, 0, 1, ev, cap, ctypes.byref(n), GPU))),
                ("scan_host", lambda: check(L.nvl_log_scan(img.ctypes.data, nbytes, 0, 1, ev, cap, ctypes.byref(n), HOST))),
            )
            for name, fn in legs:
                r = reps if mib <= 64 else max(3, reps // 3)
                t, tmin, cpu = timed(fn, r)
                d = dict(base, op="log_scan", leg=name, ms=round(t * 1e3, 3), min_ms=round(tmin * 1e3, 3),
                         GiBps=round(gib / t, 2), cpu_s_per_GiB=round(cpu / gib, 4), reps=r)
                if name == "dev":  # HIP events around the device work of one call
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ts = []
                    for _ in range(r):
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        ts.append(e0.elapsed_time(e1))
                    d["event_ms"] = round(float(np.median(ts)), 3)
                emit(d)
            # the parse path alone beside a plain read of the same bytes
            sink = torch.zeros(64, dtype=torch.int32, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def ev_time(fn, reps):
                fn(); fn()
                ts = []
                for _ in range(reps):
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1))
                return float(np.median(ts))

            def parse_only():
                rc = L.nvl_log_scan_dev(dimg.data_ptr(), nbytes, 0, 0, None, 0, ctypes.byref(n), sptr)
                assert rc == 0 and n.value == want, (rc, n.value)
            tp = ev_time(parse_only, reps)
            tr = ev_time(lambda: L.nvl_crc32c_read_probe(dimg.data_ptr(), nbytes, sink.data_ptr(), sptr), reps)
            emit(dict(base, op="log_parse_path", ms=round(tp, 3), GiBps=round(gib / (tp / 1e3), 1),
                      read_probe_ms=round(tr, 3), read_probe_GiBps=round(gib / (tr / 1e3), 1),
                      what="nvl_log_scan_dev, checksum = 0, count only: the parse kernel, both scans, the verdict "
                           "kernel and two host round trips per 64 MiB window (the parse kernel alone was not timed)"))
            assert L.nvl_crc32c_host_unregister(img.ctypes.data) == 0
            del dimg


def written_log(mib, payload, seed=12):
    """A log of mib MiB as log::Writer lays it out (db/log_writer.cc:36-82):
    logical records of `payload` bytes back to back, split into FIRST / MIDDLE
    / LAST fragments at the block ends.  Built as one chunk of up to 64 MiB
    whose last record ends exactly at the chunk's end, repeated.  Returns
    (image, logical records, fragments)."""
    total = int(mib * 2**20)
    chunk = min(total, 64 << 20)
    hdr, lens, types = [], [], []
    pos = nrec = 0
    while pos < chunk:
        left = payload
        if chunk - pos < 2 * (payload + 7 * (payload // 32761 + 2)):  # the chunk's last record: whatever fits
            left = -1
        begin = True
        while True:
            room = 32768 - pos % 32768
            if room < 7:
                pos += room
                continue
            if left < 0:  # fill to the end of the chunk, fragment by fragment
                n = room - 7
                end = pos + 7 + n >= chunk
            else:
                n = min(left, room - 7)
                left -= n
                end = left == 0
            hdr.append(pos)
            lens.append(n)
            types.append(1 if begin and end else 2 if begin else 4 if end else 3)
            pos += 7 + n
            begin = False
            if end:
                break
        nrec += 1
    assert pos == chunk, (pos, chunk)
    reps_ = total // chunk
    rng = np.random.default_rng(seed)
    one = rng.integers(0, 256, chunk, dtype=np.uint8)
    h = np.array(hdr, dtype=np.int64)
    ln = np.array(lens, dtype=np.int64)
    one[h + 4] = ln & 0xFF
    one[h + 5] = ln >> 8
    one[h + 6] = np.array(types, dtype=np.uint8)
    # block trailers are zero
    ends = h + 7 + ln
    gap = np.nonzero((ends % 32768) > 32768 - 7)[0]
    for g in gap:
        one[ends[g]:(ends[g] // 32768 + 1) * 32768] = 0
    img = np.tile(one, reps_)
    hh = (np.arange(reps_, dtype=np.uint64)[:, None] * np.uint64(chunk) + h.astype(np.uint64)[None, :]).ravel()
    rc = L.nvl_log_seal(img.ctypes.data, img.size, hh.ctypes.data, hh.size, GPU)
    assert rc == 0, rc
    return img, nrec * reps_, hh.size


def log_read_legs(sizes, reps, rounds):
    """Per image, `rounds` alternating rounds of
      read_dev       nvl_log_read_dev, payload in HBM
      read_dev_host  nvl_log_read_dev, NVL_LOG_PAYLOAD_HOST
      scan_dev       nvl_log_scan_dev (the parent's code: the difference is the record pass and the gather)
      copy_then_host the image copied to the host, then shims::LogReader's ReadRecord loop, NVL_FRAMING_HOST
                     (the parent's code: what a caller of an HBM-resident log had to do)
    each timed as the median of `reps` calls; then the median and the spread of the rounds' medians.  Then the
    gather against a device-to-device copy of the same bytes (HIP events)."""
    import subprocess
    native = os.path.join(ROOT, "tests", "native")
    subprocess.run(["make", "-s", "-C", native, "-f", "log_read.mk", "liblog_read_harness.so"], check=True)
    H = ctypes.CDLL(os.path.join(native, "liblog_read_harness.so"))
    H.shim_log_read_count.restype = ctypes.c_int
    H.shim_log_read_count.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32,
                                      ctypes.c_void_p, ctypes.c_void_p]
    for mib in sizes:
        for payload, shape in ((100, "100B"), (1024, "1KiB"), (100 * 1024, "32KiB")):
            if shape not in a.log_shapes.split(","):
                continue
            img, nrec, nfrag = written_log(mib, payload)
            nbytes = img.size
            gib = nbytes / 2**30
            dimg = torch.from_numpy(img).to("cuda")
            tot = _lib.LogReadTotals()
            assert L.nvl_log_read_dev(dimg.data_ptr(), nbytes, 0, 1, None, 0, None, 0, None, 0, ctypes.byref(tot), 0,
                                      sptr) == 0
            assert (tot.n_records, tot.n_reports) == (nrec, 0), (tot.n_records, tot.n_reports, nrec)
            pbytes = tot.payload_bytes
            base = {"log_bytes": nbytes, "records": nrec, "fragments": nfrag, "payload_bytes": pbytes, "shape": shape,
                    "op": "log_read"}
            rec = (_lib.LogRecord * nrec)()
            rp = (_lib.LogReport * 1)()
            dpay = torch.empty(pbytes, dtype=torch.uint8, device="cuda")
            hpay = np.empty(pbytes, dtype=np.uint8)
            himg = np.empty(nbytes, dtype=np.uint8)
            cap = nfrag + nbytes // 32768 + 4
            ev = (_lib.LogEvent * cap)()
            n = ctypes.c_size_t(0)
            cr, cb = ctypes.c_uint64(0), ctypes.c_uint64(0)
            torch.cuda.synchronize()

            def read_dev():
                assert L.nvl_log_read_dev(dimg.data_ptr(), nbytes, 0, 1, dpay.data_ptr(), pbytes, rec, nrec, rp, 1,
                                          ctypes.byref(tot), 0, sptr) == 0

            def read_dev_host():
                assert L.nvl_log_read_dev(dimg.data_ptr(), nbytes, 0, 1, hpay.ctypes.data, pbytes, rec, nrec, rp, 1,
                                          ctypes.byref(tot), _lib.LOG_PAYLOAD_HOST, sptr) == 0

            def scan_dev():
                assert L.nvl_log_scan_dev(dimg.data_ptr(), nbytes, 0, 1, ev, cap, ctypes.byref(n), sptr) == 0

            def copy_then_host():
                torch.from_numpy(himg).copy_(dimg)
                assert H.shim_log_read_count(himg.ctypes.data, nbytes, 1, 0, HOST, ctypes.byref(cr),
                                             ctypes.byref(cb)) == 0
                assert (cr.value, cb.value) == (nrec, pbytes)

            legs = (("read_dev", read_dev), ("read_dev_host", read_dev_host), ("scan_dev", scan_dev),
                    ("copy_then_host", copy_then_host))
            r = reps if mib <= 64 else max(3, reps // 3)
            meds = {name: [] for name, _ in legs}
            for rnd in range(rounds):
                for name, fn in legs:
                    k = r if name != "copy_then_host" else max(1, r // 3)
                    fn()
                    ts = []
                    for _ in range(k):
                        t0 = time.perf_counter()
                        fn()
                        ts.append(time.perf_counter() - t0)
                    meds[name].append(float(np.median(ts)))
                    emit(dict(base, leg=name, round=rnd, ms=round(meds[name][-1] * 1e3, 3), reps=k))
            assert hpay.tobytes() == dpay.cpu().numpy().tobytes()
            for name, _ in legs:
                m = np.array(meds[name])
                emit(dict(base, leg=name, summary=True, ms=round(float(np.median(m)) * 1e3, 3),
                          spread_ms=[round(float(m.min()) * 1e3, 3), round(float(m.max()) * 1e3, 3)],
                          GiBps=round(gib / float(np.median(m)), 2), rounds=rounds))
            # the gather beside a plain copy of the same bytes: read_dev minus the totals-only call (the scan,
            # both record scans and the totals round trip, no emit and no gather) bounds emit + gather + D2H of
            # the records from above; the device-to-device copy of the payload bytes is the floor of a gather
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def ev_time(fn, k):
                fn(); fn()
                ts = []
                for _ in range(k):
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1))
                return float(np.median(ts))

            def totals_only():
                assert L.nvl_log_read_dev(dimg.data_ptr(), nbytes, 0, 1, None, 0, None, 0, None, 0, ctypes.byref(tot),
                                          0, sptr) == 0
            src = torch.empty(pbytes, dtype=torch.uint8, device="cuda")
            t_full, t_tot = ev_time(read_dev, r), ev_time(totals_only, r)
            t_copy = ev_time(lambda: dpay.copy_(src), r)
            emit(dict(base, leg="gather_vs_copy", read_dev_event_ms=round(t_full, 3), totals_only_event_ms=round(t_tot, 3),
                      emit_gather_d2h_ms=round(t_full - t_tot, 3), d2d_copy_ms=round(t_copy, 3),
                      d2d_copy_GiBps=round(pbytes / 2**30 / (t_copy / 1e3), 1),
                      gather_bound_GiBps=round(pbytes / 2**30 / (max(t_full - t_tot, 1e-6) / 1e3), 1),
                      what="emit_gather_d2h_ms = read_dev - totals-only call: the emit kernel, the gather kernel and "
                           "the copy of the records to the host together; the gather alone is faster than that"))
            del dimg, dpay, src


if a.log_read:
    log_read_legs([float(x) for x in a.log_read.split(",")], a.reps, a.rounds)
    sys.exit(0)

if a.log_scan:
    log_scan_legs([float(x) for x in a.log_scan.split(",")], a.reps)
    sys.exit(0)

for mib in [float(x) for x in a.sizes.split(",")]:
    nblocks = max(1, int(mib * 2**20 / 4101))
    img = bench.build_table_image(nblocks)
    nbytes = len(img)
    hd = np.ascontiguousarray(table_handles(nbytes, nblocks))
    buf = bytearray(img)
    cbuf = (ctypes.c_char * len(buf)).from_buffer(buf)
    base = {"table_bytes": nbytes, "data_blocks": nblocks}
    for eng, fl in (("gpu", GPU), ("host", HOST)):
        t, tmin = med(lambda: L.nvl_sstable_seal_trailers(cbuf, len(buf), hd.ctypes.data, nblocks, fl), a.reps)
        emit(dict(base, op="seal", engine=eng, ms=round(t * 1e3, 4), min_ms=round(tmin * 1e3, 4),
                  GiBps=round(nbytes / t / 2**30, 2)))
    cap = nblocks + 2
    arr = (_lib.TableBlock * cap)()
    n, st, nb = ctypes.c_size_t(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
    for eng, fl in (("gpu", GPU), ("host", HOST)):
        def run(fl=fl):
            rc = L.nvl_sstable_verify_table(img, nbytes, arr, cap, ctypes.byref(n), ctypes.byref(st),
                                            ctypes.byref(nb), fl)
            assert rc == 0 and st.value == 0 and nb.value == 0, (rc, st.value, nb.value)
        t, tmin = med(run, a.reps)
        emit(dict(base, op="verify", engine=eng, ms=round(t * 1e3, 4), min_ms=round(tmin * 1e3, 4),
                  GiBps=round(nbytes / t / 2**30, 2)))
    dimg = torch.frombuffer(bytearray(img), dtype=torch.uint8).to("cuda")

    def run_dev():
        rc = L.nvl_sstable_verify_table_dev(dimg.data_ptr(), nbytes, arr, cap, ctypes.byref(n), ctypes.byref(st),
                                            ctypes.byref(nb), sptr)
        assert rc == 0 and st.value == 0 and nb.value == 0, (rc, st.value, nb.value)
    t, tmin = med(run_dev, a.reps)
    emit(dict(base, op="verify_dev", engine="gpu", ms=round(t * 1e3, 4), min_ms=round(tmin * 1e3, 4),
              GiBps=round(nbytes / t / 2**30, 2)))
    del dimg
    if mib == 2:
        w = np.ascontiguousarray(hd[:min(64, nblocks)])
        v = np.zeros(len(w), dtype=np.uint8)
        for eng, fl in (("gpu", GPU), ("host", HOST)):
            t, tmin = med(lambda: L.nvl_sstable_verify_blocks(img, nbytes, w.ctypes.data, len(w), v.ctypes.data,
                                                              None, fl), a.reps)
            emit({"op": "window64", "engine": eng, "blocks": len(w), "bytes": int(w[:, 1].sum()),
                  "ms": round(t * 1e3, 4), "min_ms": round(tmin * 1e3, 4)})
        try:  # the reference TableBuilder through BatchingWritableFile, sealed at Close
            import oracle
            rt = oracle.ref_table(deferred=True)
            rng = np.random.default_rng(5)
            nk = int(2**21 / 120)
            keys = [b"key%013d" % i for i in range(nk)]
            vals = [rng.integers(0, 256, 100, dtype=np.uint8).tobytes() for _ in range(nk)]
            for eng, fl in (("gpu", GPU), ("host", HOST)):
                t, tmin = med(lambda: rt.build(keys, vals, via_shim=1, seal_flags=fl), max(3, a.reps // 3))
                img2, _ = rt.build(keys, vals, via_shim=1, seal_flags=fl)
                emit({"op": "seal_tb", "engine": eng, "table_bytes": len(img2), "ms": round(t * 1e3, 3),
                      "min_ms": round(tmin * 1e3, 3), "seals": rt.seals,
                      "what": "whole reference TableBuilder build (-O0 reference objects) incl. the Close seal"})
        except Exception as e:  # noqa: BLE001 -- the builder leg needs the shipped reference build
            emit({"op": "seal_tb", "error": repr(e)})
        # 10-record MANIFEST batch: VersionEdit records of ~100-300 bytes
        rng = np.random.default_rng(9)
        recs = [rng.integers(0, 256, int(rng.integers(100, 300)), dtype=np.uint8).tobytes() for _ in range(10)]
        image, offs = bytearray(), []
        for r_ in recs:
            offs.append(len(image))
            image += bytes(7) + r_
            image[offs[-1] + 4:offs[-1] + 6] = len(r_).to_bytes(2, "little")
            image[offs[-1] + 6] = 1
        ho = np.array(offs, dtype=np.uint64)
        cimg = (ctypes.c_char * len(image)).from_buffer(image)
        for eng, fl in (("gpu", GPU), ("host", HOST)):
            t, tmin = med(lambda: L.nvl_log_seal(cimg, len(image), ho.ctypes.data, len(ho), fl), a.reps)
            emit({"op": "manifest10", "engine": eng, "bytes": len(image), "ms": round(t * 1e3, 4),
                  "min_ms": round(tmin * 1e3, 4)})
    del cbuf
