"""Python view of the call-site shims (include/nvl_framing.h): SSTable block
trailers, block and whole-table verification, log scan and log sealing, each
one CRC batch: by default the library's size policy picks the calling
thread's host CRC or the GPU (nvl_framing_uses_gpu);
``host=True`` forces the host CRC, ``host=False`` the GPU.

Verdicts carry the reference's Status texts, so a caller can report them the
way LevelDB does:

* ReadBlock, table/format.cc:65-98 -- "truncated block read",
  "block checksum mismatch", "bad block type";
* Table::Open, table/table.cc:38-82, and Block::Iter, table/block.cc --
  "file is too short to be an sstable", "not an sstable (bad magic number)",
  "bad block handle", "bad block contents", "bad entry in block";
* log::Reader::ReadPhysicalRecord, db/log_reader.cc:199-281 -- the per-record
  outcomes of nvl_log_scan;
* log::Reader::ReadRecord, db/log_reader.cc:62-175 -- the corruption reports
  of nvl_log_read / nvl_log_read_dev (LOG_REASON_TEXT).

Every function raises :class:`FramingError` on a non-OK return code; there is
no silent fallback (without a GPU the device mode raises).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, List, Sequence, Tuple, Union

import numpy as np

from . import _lib

BytesLike = Union[bytes, bytearray, memoryview, np.ndarray]

BLOCK_TEXT = {
    _lib.BLOCK_OK: "OK",
    _lib.BLOCK_TRUNCATED: "Corruption: truncated block read",
    _lib.BLOCK_CHECKSUM_MISMATCH: "Corruption: block checksum mismatch",
    _lib.BLOCK_BAD_TYPE: "Corruption: bad block type",
    _lib.BLOCK_BAD_HANDLE: "Corruption: bad block handle",
}
TABLE_TEXT = {
    _lib.TABLE_OK: "OK",
    _lib.TABLE_TOO_SHORT: "Corruption: file is too short to be an sstable",
    _lib.TABLE_BAD_MAGIC: "Corruption: not an sstable (bad magic number)",
    _lib.TABLE_BAD_FOOTER: "Corruption: bad block handle",
    _lib.TABLE_INDEX_UNREADABLE: "index block unreadable",  # blocks[0] carries the ReadBlock text
    _lib.TABLE_BAD_INDEX_BLOCK: "Corruption: bad block contents",
    _lib.TABLE_BAD_INDEX_ENTRY: "Corruption: bad entry in block",
    _lib.TABLE_COMPRESSED_INDEX: "index block is compressed (not parsed)",
}
ROLE_TEXT = {_lib.TBLOCK_INDEX: "index", _lib.TBLOCK_METAINDEX: "metaindex", _lib.TBLOCK_META: "meta",
             _lib.TBLOCK_DATA: "data"}


class FramingError(RuntimeError):
    def __init__(self, rc: int, what: str):
        super().__init__(f"{what}: {_lib.lib.nvl_crc32c_strerror(rc).decode()} ({rc})")
        self.rc = rc


def _flags(host) -> int:
    """host=None: the library's size policy (nvl_framing_uses_gpu); True: the
    host CRC; False: the GPU whatever the size."""
    if host is None:
        return 0
    return _lib.FRAMING_HOST if host else _lib.FRAMING_GPU


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise FramingError(rc, what)


def _handles(handles) -> np.ndarray:
    h = np.ascontiguousarray(np.asarray(handles, dtype=np.uint64).reshape(-1, 2))
    return h


def _ro(data: BytesLike):
    if isinstance(data, np.ndarray):
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        return a.ctypes.data, a.size, a
    if isinstance(data, memoryview):
        data = data.tobytes()
    if isinstance(data, bytearray):
        return (ctypes.c_char * len(data)).from_buffer(data), len(data), data
    return data, len(data), data


def seal_trailers(image: Union[bytearray, np.ndarray], handles, *, host: Optional[bool] = None) -> None:
    """TableBuilder::WriteRawBlock's trailer (table/table_builder.cc:183-188) for
    every (offset, size) handle, in place: image[off+size] holds the type,
    Mask(Value(block | type)) goes to image[off+size+1 .. +5)."""
    h = _handles(handles)
    if isinstance(image, np.ndarray):
        ptr, n = image.ctypes.data, image.nbytes
    elif isinstance(image, bytearray):
        ptr, n = (ctypes.c_char * len(image)).from_buffer(image), len(image)
    else:
        raise TypeError("seal_trailers writes in place: pass a bytearray or a numpy array")
    _check(_lib.lib.nvl_sstable_seal_trailers(ptr, n, h.ctypes.data, len(h), _flags(host)), "seal_trailers")


def verify_blocks(image: BytesLike, handles, *, host: Optional[bool] = None) -> np.ndarray:
    """ReadBlock's checks (verify_checksums) for every handle: an array of
    NVL_BLOCK_* verdicts (see BLOCK_TEXT)."""
    h = _handles(handles)
    ptr, n, _keep = _ro(image)
    v = np.zeros(len(h), dtype=np.uint8)
    bad = ctypes.c_uint64(0)
    _check(_lib.lib.nvl_sstable_verify_blocks(ptr, n, h.ctypes.data, len(h), v.ctypes.data, ctypes.byref(bad),
                                              _flags(host)), "verify_blocks")
    return v


@dataclass
class TableBlockReport:
    offset: int
    size: int
    role: str
    verdict: int

    @property
    def text(self) -> str:
        return BLOCK_TEXT[self.verdict]


@dataclass
class TableReport:
    status: int
    blocks: List[TableBlockReport]

    @property
    def ok(self) -> bool:
        return self.status == _lib.TABLE_OK and all(b.verdict == _lib.BLOCK_OK for b in self.blocks)

    @property
    def status_text(self) -> str:
        if self.status == _lib.TABLE_INDEX_UNREADABLE and self.blocks:
            return self.blocks[0].text
        return TABLE_TEXT[self.status]

    def bad(self) -> List[TableBlockReport]:
        return [b for b in self.blocks if b.verdict != _lib.BLOCK_OK]


def verify_table(image: BytesLike, *, host: Optional[bool] = None) -> TableReport:
    """Every block of an SSTable image verified in one batch
    (nvl_sstable_verify_table): index, metaindex, meta blocks, data blocks."""
    ptr, n, _keep = _ro(image)
    cnt = ctypes.c_size_t(0)
    st = ctypes.c_uint32(0)
    bad = ctypes.c_uint64(0)
    # one call when the guess fits: the index holds at most one handle per 3+2 bytes
    cap = max(16, min(n // 5 + 8, 1 << 22))
    while True:
        arr = (_lib.TableBlock * cap)()
        rc = _lib.lib.nvl_sstable_verify_table(ptr, n, arr, cap, ctypes.byref(cnt), ctypes.byref(st),
                                               ctypes.byref(bad), _flags(host))
        if rc == _lib.ENOSPC and cnt.value > cap:
            cap = cnt.value
            continue
        _check(rc, "verify_table")
        break
    blocks = [TableBlockReport(a.offset, a.size, ROLE_TEXT[a.role], a.verdict) for a in arr[:cnt.value]]
    return TableReport(st.value, blocks)


def verify_table_dev(image, stream=None) -> TableReport:
    """verify_table for an SSTable image already in device memory: a 1-D
    uint8 torch tensor on the GPU (nvl_sstable_verify_table_dev; only the
    footer, index and metaindex come back to the host)."""
    import torch
    if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dtype == torch.uint8 and image.dim() == 1
            and image.is_contiguous()):
        raise TypeError("verify_table_dev: a contiguous 1-D uint8 tensor on the GPU")
    st_ = torch.cuda.current_stream(image.device).cuda_stream if stream is None else stream
    n = image.numel()
    cnt = ctypes.c_size_t(0)
    st = ctypes.c_uint32(0)
    bad = ctypes.c_uint64(0)
    with torch.cuda.device(image.device):
        _check(_lib.lib.nvl_sstable_verify_table_dev(image.data_ptr(), n, None, 0, ctypes.byref(cnt), ctypes.byref(st),
                                                     ctypes.byref(bad), st_), "verify_table_dev")
        cap = max(cnt.value, 1)
        arr = (_lib.TableBlock * cap)()
        _check(_lib.lib.nvl_sstable_verify_table_dev(image.data_ptr(), n, arr, cap, ctypes.byref(cnt), ctypes.byref(st),
                                                     ctypes.byref(bad), st_), "verify_table_dev")
    blocks = [TableBlockReport(a.offset, a.size, ROLE_TEXT[a.role], a.verdict) for a in arr[:cnt.value]]
    return TableReport(st.value, blocks)


LOG_KIND = {_lib.LOG_RECORD: "record", _lib.LOG_BAD_LENGTH: "bad record length",
            _lib.LOG_CHECKSUM: "checksum mismatch", _lib.LOG_ZERO: "zero", _lib.LOG_EOF: "eof"}


def _log_events(scan, n: int, what: str) -> List[Tuple[str, int, int, int]]:
    """scan(events, cap, count_ref) -> rc, called until the events fit."""
    cnt = ctypes.c_size_t(0)
    # One scan when the guess fits (records of >= ~256 B on average); a log of
    # tinier records is scanned again with the exact count the first call reported.
    cap = n // 256 + 64
    while True:
        ev = (_lib.LogEvent * cap)()
        rc = scan(ev, cap, ctypes.byref(cnt))
        if rc == _lib.ENOSPC and cnt.value > cap:
            cap = cnt.value
            continue
        _check(rc, what)
        break
    return [(LOG_KIND[e.kind], e.offset, e.length, e.type) for e in ev[:cnt.value]]


def log_scan(image: BytesLike, *, start: int = 0, checksum: bool = True, host: Optional[bool] = None,
             device_parse: bool = False) -> List[Tuple[str, int, int, int]]:
    """ReadPhysicalRecord's outcomes over a log image (nvl_log_scan):
    [(kind, header_offset, payload_length, type)] ending with ("eof", ...).
    ``device_parse=True``: the bytes go to the GPU once and the headers are
    parsed there as well (nvl_log_scan_staged; always the GPU, so not with
    ``host=True``)."""
    ptr, n, _keep = _ro(image)
    if device_parse:
        if host:
            raise ValueError("log_scan: device_parse runs on the GPU (host=True contradicts it)")
        return _log_events(lambda ev, cap, cnt: _lib.lib.nvl_log_scan_staged(ptr, n, start, int(checksum), ev, cap, cnt),
                           n, "log_scan(device_parse)")
    return _log_events(lambda ev, cap, cnt: _lib.lib.nvl_log_scan(ptr, n, start, int(checksum), ev, cap, cnt,
                                                                  _flags(host)), n, "log_scan")


def log_scan_dev(image, *, start: int = 0, checksum: bool = True, stream=None) -> List[Tuple[str, int, int, int]]:
    """log_scan for a log image already in device memory: a contiguous 1-D
    uint8 torch tensor on the GPU (nvl_log_scan_dev: parsed, checked and
    replayed there; only the events come back)."""
    import torch
    if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dtype == torch.uint8 and image.dim() == 1
            and image.is_contiguous()):
        raise TypeError("log_scan_dev: a contiguous 1-D uint8 tensor on the GPU")
    st_ = torch.cuda.current_stream(image.device).cuda_stream if stream is None else stream
    n = image.numel()
    with torch.cuda.device(image.device):
        return _log_events(lambda ev, cap, cnt: _lib.lib.nvl_log_scan_dev(image.data_ptr(), n, start, int(checksum),
                                                                          ev, cap, cnt, st_), n, "log_scan_dev")


LOG_REASON_TEXT = {
    _lib.LOG_REASON_BAD_LENGTH: "bad record length",
    _lib.LOG_REASON_CHECKSUM: "checksum mismatch",
    _lib.LOG_REASON_PARTIAL_1: "partial record without end(1)",
    _lib.LOG_REASON_PARTIAL_2: "partial record without end(2)",
    _lib.LOG_REASON_MISSING_START_1: "missing start of fragmented record(1)",
    _lib.LOG_REASON_MISSING_START_2: "missing start of fragmented record(2)",
    _lib.LOG_REASON_IN_MIDDLE: "error in middle of record",
    _lib.LOG_REASON_UNKNOWN_TYPE: "unknown record type %u",
}
LOG_RECORD_DTYPE = np.dtype([("offset", "<u8"), ("payload", "<u8"), ("length", "<u8"), ("fragments", "<u4"),
                             ("reports_before", "<u4")])
LOG_REPORT_DTYPE = np.dtype([("bytes", "<u8"), ("reason", "<u4"), ("type", "<u4")])


@dataclass
class LogRead:
    """What log::Reader::ReadRecord returns over a log image, in reader order:
    ``records`` (LOG_RECORD_DTYPE; ``reports_before`` interleaves them with
    the reports), ``reports`` as (bytes, reason text) with the reference's
    strings, and the records' bytes packed in ``payload`` (bytes, or a CUDA
    tensor from :func:`log_read_dev`)."""
    records: np.ndarray
    reports: List[Tuple[int, str]]
    payload: object

    def record_bytes(self, k: int) -> bytes:
        r = self.records[k]
        part = self.payload[int(r["payload"]):int(r["payload"]) + int(r["length"])]
        return bytes(part) if isinstance(part, (bytes, bytearray, memoryview)) else part.cpu().numpy().tobytes()


def _log_read(read, n: int, make_payload, what: str) -> LogRead:
    """read(payload_ptr, payload_cap, records, rec_cap, reports, rep_cap, totals) -> rc: the totals first, then
    one call with exact capacities."""
    tot = _lib.LogReadTotals()
    _check(read(None, 0, None, 0, None, 0, ctypes.byref(tot)), what)
    nrec, nrep, nbytes = tot.n_records, tot.n_reports, tot.payload_bytes
    records = np.zeros(max(nrec, 1), dtype=LOG_RECORD_DTYPE)
    reports = np.zeros(max(nrep, 1), dtype=LOG_REPORT_DTYPE)
    payload, ptr = make_payload(max(nbytes, 1))
    _check(read(ptr, nbytes, records.ctypes.data, nrec, reports.ctypes.data, nrep, ctypes.byref(tot)), what)
    texts = [(int(r["bytes"]), LOG_REASON_TEXT[int(r["reason"])].replace("%u", str(int(r["type"]))))
             for r in reports[:nrep]]
    return LogRead(records[:nrec], texts, payload[:nbytes])


def log_read(image: BytesLike, *, initial_offset: int = 0, checksum: bool = True,
             host: Optional[bool] = None) -> LogRead:
    """ReadRecord's logical records and corruption reports over a host log
    image read from ``initial_offset`` (nvl_log_read: the physical scan of
    :func:`log_scan` under ``host``, then the record rules)."""
    ptr, n, _keep = _ro(image)

    def make(nbytes):
        buf = np.zeros(nbytes, dtype=np.uint8)
        return buf, buf.ctypes.data

    got = _log_read(lambda p, pc, r, rc_, q, qc, t: _lib.lib.nvl_log_read(ptr, n, initial_offset, int(checksum), p, pc,
                                                                       r, rc_, q, qc, t, _flags(host)),
                    n, make, "log_read")
    got.payload = got.payload.tobytes()
    return got


def log_read_dev(image, *, initial_offset: int = 0, checksum: bool = True, stream=None) -> LogRead:
    """log_read for a log image already in device memory: a contiguous 1-D
    uint8 torch tensor on the GPU (nvl_log_read_dev: scanned, joined and
    gathered there).  ``payload`` is a tensor on the image's device."""
    import torch
    if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dtype == torch.uint8 and image.dim() == 1
            and image.is_contiguous()):
        raise TypeError("log_read_dev: a contiguous 1-D uint8 tensor on the GPU")
    st_ = torch.cuda.current_stream(image.device).cuda_stream if stream is None else stream
    n = image.numel()

    def make(nbytes):
        buf = torch.empty(nbytes, dtype=torch.uint8, device=image.device)
        return buf, buf.data_ptr()

    with torch.cuda.device(image.device):
        return _log_read(lambda p, pc, r, rc_, q, qc, t: _lib.lib.nvl_log_read_dev(
            image.data_ptr(), n, initial_offset, int(checksum), p, pc, r, rc_, q, qc, t, 0, st_), n, make,
            "log_read_dev")


def log_seal(image: Union[bytearray, np.ndarray], header_offsets: Sequence[int], *, host: Optional[bool] = None) -> None:
    """log::Writer's header CRCs (db/log_writer.cc:93-97) for every header offset, in place."""
    off = np.ascontiguousarray(np.asarray(header_offsets, dtype=np.uint64))
    if isinstance(image, np.ndarray):
        ptr, n = image.ctypes.data, image.nbytes
    elif isinstance(image, bytearray):
        ptr, n = (ctypes.c_char * len(image)).from_buffer(image), len(image)
    else:
        raise TypeError("log_seal writes in place: pass a bytearray or a numpy array")
    _check(_lib.lib.nvl_log_seal(ptr, n, off.ctypes.data, len(off), _flags(host)), "log_seal")
