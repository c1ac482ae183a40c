// nvlevelz_amd/csrc/crc32c_log_core.h -- the log reader's block rules
// (ReadPhysicalRecord, db/log_reader.cc:199-266), written once for the host
// scan (nvl_log_scan, crc32c_framing.cpp) and the kernels of nvl_log_scan_dev
// / nvl_log_scan_staged (crc32c_log_dev.hip).  log::Reader restarts its parse
// at every 32 KiB block (:199-218), so each block is taken on its own: its
// headers are walked as if every record passed its checksum, the candidates'
// CRCs are computed in one batch, and the block is replayed up to its first
// mismatch (`cut`; count: none).  No STL, no HIP headers.  Internal.
#pragma once
#include "crc32c_math.h"
#include "nvl_framing.h"

namespace nvl {

constexpr uint32_t kLogBlk = NVL_LOG_BLOCK_SIZE, kLogHdr = NVL_LOG_HEADER_SIZE;
constexpr uint32_t kLogSlab = 4682;            // positions kept per block: it holds at most 4681 records of 7 bytes
constexpr uint32_t kLogNoClose = 0xFFFFFFFFu;  // LogBlockInfo::close_kind: the block trailer was skipped

struct LogBlockInfo {
  uint32_t count;       // candidate records
  uint32_t close_kind;  // NVL_LOG_BAD_LENGTH / ZERO / EOF, or kLogNoClose
  uint32_t close_pos;   // where the walk stopped (in the block): the closing event's place
  uint32_t m;           // block bytes (< 32768: the short last block, where the input ends)
};
struct LogSlot { uint32_t off, len; };  // a candidate in the CRC batch: offset in the block, bytes

// The entry points' argument check (false: NVL_CRC32C_EINVAL); *n_events is zero on every error return.
inline bool log_scan_args(const void* data, uint64_t len, uint64_t start, size_t* n_events) {
  if (n_events) *n_events = 0;
  return (data || !len) && n_events && (start % kLogBlk) == 0;
}

// ReadPhysicalRecord's header checks (:203-252) over the block b[0, m), m <=
// 32768; pos[k] = candidate k's position (at most 32761, kLogSlab entries are
// enough).  log::Reader reads kBlockSize at a time; a short read (incl. 0
// bytes) marks EOF (:205-218).
NVL_HD inline LogBlockInfo log_walk_block(const uint8_t* b, uint32_t m, uint16_t* pos) {
  const bool eof = m < kLogBlk;
  uint32_t at = 0, count = 0, kind = kLogNoClose;
  while (true) {
    if (m - at < kLogHdr) {
      if (eof) kind = NVL_LOG_EOF;  // empty, or a truncated header at the end of the file: EOF, not a corruption
      break;                        // otherwise the block trailer is skipped
    }
    const uint32_t length = (uint32_t)b[at + 4] | ((uint32_t)b[at + 5] << 8), type = b[at + 6];
    if (kLogHdr + length > m - at) {
      kind = eof ? NVL_LOG_EOF : NVL_LOG_BAD_LENGTH;  // :234-244
      break;
    }
    if (type == 0 && length == 0) {  // :246-252
      kind = NVL_LOG_ZERO;
      break;
    }
    pos[count++] = (uint16_t)at;
    at += kLogHdr + length;
  }
  return LogBlockInfo{count, kind, at, m};
}

// Value(header + 6, 1 + length): type | payload (:256-257).  Candidate k ends
// at the next position or where the walk stopped: the image is not read again.
NVL_HD inline LogSlot log_slot(const LogBlockInfo& bi, const uint16_t* pos, uint32_t k) {
  const uint32_t at = pos[k], next = k + 1u < bi.count ? (uint32_t)pos[k + 1u] : bi.close_pos;
  return LogSlot{at + 6u, next - at - 6u};
}

// Does candidate k's CRC match Unmask(its header's stored value) (:254-257)?
NVL_HD inline bool log_crc_ok(const uint8_t* b, const uint16_t* pos, uint32_t k, uint32_t crc) {
  const uint8_t* h = b + pos[k];
  return crc == unmask((uint32_t)h[0] | ((uint32_t)h[1] << 8) | ((uint32_t)h[2] << 16) | ((uint32_t)h[3] << 24));
}

// Replay: the block emits records [0, cut), then its tail events.  Record k
// of the block b; f0 = the file offset of b[0].
NVL_HD inline nvl_log_event log_record_event(const LogBlockInfo& bi, const uint16_t* pos, uint32_t k,
                                             const uint8_t* b, uint64_t f0) {
  const LogSlot s = log_slot(bi, pos, k);
  return nvl_log_event{f0 + pos[k], f0 + bi.m, s.len - 1u, b[s.off], NVL_LOG_RECORD, 0u};
}

// The zero, one or two tail events, in order, each handed to put(event): a
// block cut at candidate `cut` reports the mismatch there and drops the rest
// of its buffer (:258-266), an uncut one ends with its closing event, if any.
// When that empties the short last block before its end was reported, the
// next read finds nothing: one more EOF.
template <class Put>
NVL_HD inline void log_tail_events(const LogBlockInfo& bi, const uint16_t* pos, uint32_t cut, uint64_t f0, Put put) {
  const uint64_t end = f0 + bi.m;
  if (cut < bi.count) put(nvl_log_event{f0 + pos[cut], end, 0u, 0u, NVL_LOG_CHECKSUM, 0u});
  else if (bi.close_kind != kLogNoClose) put(nvl_log_event{f0 + bi.close_pos, end, 0u, 0u, bi.close_kind, 0u});
  if (bi.m < kLogBlk && (cut < bi.count || bi.close_kind != NVL_LOG_EOF))
    put(nvl_log_event{end, end, 0u, 0u, NVL_LOG_EOF, 0u});
}

// The events the block emits, counted by the function that lays them out.
NVL_HD inline uint32_t log_emit_count(const LogBlockInfo& bi, const uint16_t* pos, uint32_t cut) {
  uint32_t n = cut < bi.count ? cut : bi.count;
  log_tail_events(bi, pos, cut, 0, [&n](const nvl_log_event&) { ++n; });
  return n;
}

}  // namespace nvl
