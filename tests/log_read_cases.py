"""Images and helpers shared by tests/test_log_read.py (CPU),
tests/test_log_read_dev.py (GPU) and tools/gen_log_read_golden.py: the
record-level edge images of the log reader (log::Reader::ReadRecord,
db/log_reader.cc:62-175), the dense and gather images of the device reader,
the harness trace of a result, and the two entry points as (totals, records,
reports, payload) tuples that compare with ==.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from test_log_scan_dev import BLK, HOST, Log  # noqa: E402  (the image builder)

FULL, FIRST, MIDDLE, LAST = 1, 2, 3, 4
PAYLOAD_HOST = 0x1000
REASONS = ("", "bad record length", "checksum mismatch", "partial record without end(1)",
           "partial record without end(2)", "missing start of fragmented record(1)",
           "missing start of fragmented record(2)", "error in middle of record", "unknown record type %u")


def fit(lg, n, rtype):
    """A record of n bytes placed as a writer would: never across a block end
    (the block is closed with a filler record, or zeros when < 7 bytes are left)."""
    room = BLK - len(lg.buf) % BLK
    if room < 7 + n:
        if room >= 7:
            lg.record(room - 7, FULL)
        else:
            lg.raw(bytes(room))
    return lg.record(n, rtype)


def bad_length(lg):
    """A header whose length runs past the block, then the rest of the block."""
    room = BLK - len(lg.buf) % BLK
    lg.raw(bytes(4) + (60000).to_bytes(2, "little") + b"\x01")
    return lg.garbage(room - 7)


def edge_cases():
    """[(name, image bytes, initial_offset, checksum)]: one reader rule each."""
    rng = np.random.default_rng(20250219)
    out = []

    def add(name, img, initial_offset=0, checksum=1):
        out.append((name, bytes(img), initial_offset, checksum))

    add("zero_first_then_full", Log(rng).record(0, FIRST).record(10, FULL).record(3, FULL).sealed())
    add("zero_first_then_first", Log(rng).record(0, FIRST).record(5, FIRST).record(3, LAST).sealed())
    add("first_then_first", Log(rng).record(5, FIRST).record(6, FIRST).record(2, LAST).sealed())
    add("first_then_full", Log(rng).record(5, FIRST).record(2, MIDDLE).record(4, FULL).sealed())
    add("lone_middle", Log(rng).record(3, FULL).record(4, MIDDLE).record(2, FULL).sealed())
    add("lone_last", Log(rng).record(3, FULL).record(4, LAST).record(2, FULL).sealed())
    add("unknown_outside", Log(rng).record(3, FULL).record(5, 7).record(2, FULL).sealed())
    add("unknown_inside", Log(rng).record(4, FIRST).record(6, MIDDLE).record(5, 7).record(2, LAST).sealed())
    add("type_zero_with_payload", Log(rng).record(4, FIRST).record(5, 0).record(2, FULL).sealed())
    # a checksum failure inside a fragmented record drops the rest of its block
    lg = Log(rng).record(100, FIRST).record(50, MIDDLE).record(20, LAST).fill_block(BLK).record(5, LAST).record(7, FULL)
    img = lg.sealed()
    img[107 + 7 + 10] ^= 0x04
    add("checksum_inside_fragment", img)
    add("checksum_inside_fragment_unchecked", img, 0, 0)
    add("bad_length_after_zero_first", bad_length(Log(rng).record(9, FULL).record(0, FIRST)).record(5, FULL).sealed())
    lg = Log(rng).record(9, FULL).record(0, FIRST)
    room = BLK - len(lg.buf)
    add("zero_after_zero_first", lg.raw(bytes(7)).garbage(room - 7).record(5, FULL).sealed())
    add("bad_length_inside_fragment", bad_length(Log(rng).record(8, FIRST).record(9, MIDDLE)).record(5, LAST).sealed())
    add("eof_inside_fragment", Log(rng).record(6, FULL).record(10, FIRST).record(5, MIDDLE).sealed())
    add("eof_after_zero_first", Log(rng).record(6, FULL).record(0, FIRST).sealed())
    add("truncated_last_fragment", Log(rng).record(10, FIRST).sealed() + bytes(4) + (100).to_bytes(2, "little") + b"\x04xy")
    # a record over three blocks and a half, its fragments ending exactly at the block ends
    big = Log(rng).record(20, FULL).record(BLK - 7 - 27, FIRST).record(BLK - 7, MIDDLE).record(BLK - 7, MIDDLE)
    big = big.record(100, LAST).record(50, FULL).record(0, FULL).sealed()
    add("three_blocks", big)
    for io in (1, 27, 28, BLK - 1, BLK, BLK + 1, BLK + 10, 2 * BLK, 3 * BLK, 3 * BLK + 1, 3 * BLK + 107, 3 * BLK + 108,
               len(big) - 7, len(big) - 1, len(big), len(big) + 5, 4 * BLK, 5 * BLK + 3):
        add(f"three_blocks_from_{io}", big, io)
    # initial_offset inside a block trailer: the reader starts in the next block
    lg = Log(rng).fill_block(BLK - 3).raw(b"\x01\x02\x03").record(30, LAST).record(40, FULL)
    img = lg.sealed()
    for io in (BLK - 6, BLK - 5, BLK - 3, BLK - 1):
        add(f"trailer_from_{io}", img, io)
    add("fragment_ends_block", Log(rng).fill_block(BLK - 107).record(100, FIRST).record(0, MIDDLE).record(9, LAST).sealed())
    # reports near initial_offset: the filter pos_ - bytes >= initial_offset
    lg = Log(rng).record(10, FULL).record(20, MIDDLE).record(30, LAST).record(3, 9).record(4, FULL)
    img = lg.sealed()
    for io in (1, 17, 18, 44, 45, 82):
        add(f"filter_from_{io}", img, io)
    add("empty", b"")
    add("empty_from_5", b"", 5)
    return out


_dense = {}


def dense_image(breaker=None, at=0, blocks=3):
    """`blocks` blocks of 0- and 1-byte MIDDLE fragments between a FIRST and a
    LAST (about 4681 events per block); `breaker` ("full", "unknown" or
    "bad") replaces the event at index `at`.  Returns (image, event count)."""
    if blocks not in _dense:  # the unsealed image, built once
        lg = Log(np.random.default_rng(4242))
        lg.record(1, FIRST)
        i = 1
        end = blocks * BLK
        while end - len(lg.buf) >= 7 + 16:
            room = BLK - len(lg.buf) % BLK
            if room < 7:
                lg.raw(bytes(room))
                continue
            lg.record(min(i & 1, room - 7), MIDDLE)
            i += 1
        lg.record(5, LAST).record(3, FULL)
        _dense[blocks] = lg
    base = _dense[blocks]
    lg = Log(None)
    lg.buf, lg.hdrs = bytearray(base.buf), base.hdrs
    if breaker in ("full", "unknown"):
        lg.buf[lg.hdrs[at] + 6] = FULL if breaker == "full" else 9
    img = lg.sealed()
    if breaker == "bad":
        img[lg.hdrs[at] + 2] ^= 0x20  # its stored CRC: the rest of its block is dropped
    return bytes(img), len(lg.hdrs)


def seam_positions():
    out = set()
    for k in range(1, 5):
        for tile in (64, 256, 1024):
            out.update((k * tile - 1, k * tile, k * tile + 1))
    return sorted(out)


def gather_image(pre):
    """Records whose bytes start at every alignment: `pre` bytes first, then
    whole and three-fragment records of the lengths at which the gather's
    paths change."""
    rng = np.random.default_rng(900 + pre)
    lg = Log(rng)
    lg.record(pre, FULL)
    for n in (0, 1, 15, 16, 17, 4095, 4096, 4097, 32761):
        fit(lg, n, FULL)
        fit(lg, n, FIRST)
        fit(lg, n, MIDDLE)
        fit(lg, n, LAST)
        fit(lg, pre, FULL)
    return bytes(lg.sealed())


# ------------------------------------------------------------------ results --

def _result(tot, rec, rep, payload):
    nr, nq = tot.n_records, tot.n_reports
    return ((nr, nq, tot.payload_bytes), bytes(rec)[:nr * 32], bytes(rep)[:nq * 16], payload)


def host_read(L, img, initial_offset=0, checksum=1, flags=HOST):
    """nvl_log_read: the totals query, then exact capacities."""
    tot = L.LogReadTotals()
    rc = L.lib.nvl_log_read(img, len(img), initial_offset, checksum, None, 0, None, 0, None, 0, ctypes.byref(tot), flags)
    assert rc == 0, rc
    nr, nq, nb = tot.n_records, tot.n_reports, tot.payload_bytes
    rec, rep = (L.LogRecord * max(nr, 1))(), (L.LogReport * max(nq, 1))()
    payload = ctypes.create_string_buffer(max(nb, 1))
    tot2 = L.LogReadTotals()
    rc = L.lib.nvl_log_read(img, len(img), initial_offset, checksum, payload, nb, rec, nr, rep, nq, ctypes.byref(tot2),
                            flags)
    assert rc == 0, rc
    assert (tot2.n_records, tot2.n_reports, tot2.payload_bytes) == (nr, nq, nb)
    return _result(tot, rec, rep, payload.raw[:nb])


def dev_read(L, dimg, n, initial_offset, checksum, stream, want_totals, host_payload=False, shift=0):
    """nvl_log_read_dev with capacities from want_totals into a payload buffer
    with 64 guard bytes of 0xA5 on each side (`shift` more in front), which
    must come back intact."""
    import torch
    nr, nq, nb = want_totals
    rec, rep = (L.LogRecord * max(nr, 1))(), (L.LogReport * max(nq, 1))()
    tot = L.LogReadTotals()
    lead = 64 + shift
    if host_payload:
        buf = np.full(lead + nb + 64, 0xA5, dtype=np.uint8)
        ptr = buf.ctypes.data + lead
    else:
        buf = torch.full((lead + nb + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ptr = buf.data_ptr() + lead
    rc = L.lib.nvl_log_read_dev(dimg.data_ptr() if n else None, n, initial_offset, checksum, ptr, nb, rec, nr, rep, nq,
                                ctypes.byref(tot), PAYLOAD_HOST if host_payload else 0, stream)
    assert rc == 0, rc
    raw = buf.tobytes() if host_payload else buf.cpu().numpy().tobytes()
    assert raw[:lead] == b"\xA5" * lead and raw[lead + nb:] == b"\xA5" * 64, "payload guard bytes overwritten"
    return _result(tot, rec, rep, raw[lead:lead + nb])


def render(result, crc):
    """The harness trace of a result: R <offset> <length> <crc32c>, C <bytes>
    Corruption: <reason>, interleaved by reports_before, then E."""
    (nr, nq, _nb), rec, rep, payload = result
    recs = np.frombuffer(rec, dtype=np.dtype([("offset", "<u8"), ("payload", "<u8"), ("length", "<u8"),
                                              ("fragments", "<u4"), ("reports_before", "<u4")]))
    reps = np.frombuffer(rep, dtype=np.dtype([("bytes", "<u8"), ("reason", "<u4"), ("type", "<u4")]))
    lines, r = [], 0
    for k in range(nr + 1):
        upto = int(recs[k]["reports_before"]) if k < nr else nq
        assert r <= upto <= nq
        while r < upto:
            lines.append("C %d Corruption: %s" % (reps[r]["bytes"], REASONS[reps[r]["reason"]].replace(
                "%u", str(int(reps[r]["type"])))))
            r += 1
        if k < nr:
            at, n = int(recs[k]["payload"]), int(recs[k]["length"])
            lines.append("R %d %d %d" % (recs[k]["offset"], n, crc(payload[at:at + n])))
    return "\n".join(lines + ["E"]) + "\n"


def describe(result):
    return result[0], render(result, lambda b: len(b))[:600]
