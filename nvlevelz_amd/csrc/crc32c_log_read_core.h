// nvlevelz_amd/csrc/crc32c_log_read_core.h -- the log reader's record rules
// (log::Reader::ReadRecord, db/log_reader.cc:62-175, and its report filter,
// :181-190), written once for the host loop of nvl_log_read
// (crc32c_framing.cpp) and the kernels of nvl_log_read_dev
// (crc32c_log_read.hip).  Input: the physical events of nvl_log_scan, one
// ReadPhysicalRecord outcome each.  An event is classified on its own
// (log_read_classify); what ReadRecord does with it depends on the reader's
// state -- resyncing_ (:86-95), idle, in_fragmented_record, or done: a
// ReadRecord returned false, which ends the caller's loop -- and, inside a
// fragmented record, on scratch->size().  log_read_next is the state's
// transition, a function of the event's class alone, so a run of events is a
// composition of maps on these four states (log_read_fn / log_read_compose: the
// kernels' prefix scan); log_read_step is what one event emits from a given
// state: at most one record and at most two reports.  No STL, no HIP headers.
// Internal.
#pragma once
#include "crc32c_log_core.h"
#include "nvl_framing.h"

namespace nvl {

enum : uint32_t { kLrResync = 0, kLrIdle = 1, kLrFrag = 2, kLrDone = 3 };  // the reader's state before an event
enum : uint32_t { kLcFull = 0, kLcFirst, kLcMiddle, kLcLast, kLcUnknown, kLcBad, kLcEof };

// One event as the record rules see it (16 bytes: the whole image's events
// stay in device memory across the scan's windows).
struct LogReadEvent {
  uint64_t offset;  // of the header
  uint32_t span;    // physical record: payload bytes; BAD_LENGTH / CHECKSUM / ZERO: block_end - offset
  uint8_t cls;      // kLc*
  uint8_t phys;     // NVL_LOG_REASON_BAD_LENGTH / _CHECKSUM: ReadPhysicalRecord reported it itself (:236,:264)
  uint8_t type;     // the stored type byte (kLcUnknown: "unknown record type %u")
  uint8_t rec;      // 1: a physical record (pos_ after it = offset + 7 + span), 0: pos_ = offset + span
};

// kFullType .. kLastType are 1 .. 4 (db/log_format.h:14-24).  ReadRecord
// switches on what ReadPhysicalRecord returns, a stored type byte or its own
// kEof = 5 / kBadRecord = 6 (db/log_reader.h:84-92), so a record that passed
// its checks with a stored type of 5 or 6 is taken for those; any other type
// is the switch's default (:169-178).  A record that starts before
// initial_offset is kBadRecord (:270-275), as are the three block-dropping
// outcomes; only two of those report (:236,:264).
NVL_HD inline LogReadEvent log_read_classify(const nvl_log_event& e, uint64_t initial_offset) {
  LogReadEvent r{e.offset, 0u, (uint8_t)kLcBad, 0u, (uint8_t)e.type, 0u};
  switch (e.kind) {
    case NVL_LOG_RECORD:
      r.span = e.length;
      r.rec = 1u;
      if (e.offset >= initial_offset && e.type != 6u)
        r.cls = (uint8_t)(e.type >= 1u && e.type <= 4u ? e.type - 1u : (e.type == 5u ? kLcEof : kLcUnknown));
      break;
    case NVL_LOG_BAD_LENGTH:
    case NVL_LOG_CHECKSUM:
      r.phys = (uint8_t)(e.kind == NVL_LOG_BAD_LENGTH ? NVL_LOG_REASON_BAD_LENGTH : NVL_LOG_REASON_CHECKSUM);
      r.span = (uint32_t)(e.block_end - e.offset);
      break;
    case NVL_LOG_ZERO:
      r.span = (uint32_t)(e.block_end - e.offset);
      break;
    default:
      r.cls = (uint8_t)kLcEof;
      break;
  }
  return r;
}

// Fragment bytes the event adds to a record (the scratch size inside a
// fragmented record is a difference of prefix sums of this).
NVL_HD inline uint32_t log_read_fragment_bytes(const LogReadEvent& e) { return e.cls <= kLcLast ? e.span : 0u; }

// The state after an event of class `cls`.  Resyncing swallows MIDDLE, and
// LAST (which ends it); anything else ends it and is processed as from idle
// (:86-95).  Then: FIRST opens a fragmented record (:114-129), MIDDLE keeps
// what there is (:131-138), every other class leaves none open.  kEof ends
// the read (:152-159): no later event is looked at.
NVL_HD inline uint32_t log_read_next(uint32_t state, uint32_t cls) {
  if (state == kLrDone || cls == kLcEof) return kLrDone;
  if (state == kLrResync) {
    if (cls == kLcMiddle) return kLrResync;
    if (cls == kLcLast) return kLrIdle;
    state = kLrIdle;
  }
  if (cls == kLcFirst) return kLrFrag;
  return cls == kLcMiddle ? state : (uint32_t)kLrIdle;
}

// A class's transition as a map on the four states, two bits per state; the
// composition "a, then b" (associative: the kernels scan it).
constexpr uint32_t kLogReadFnId = kLrResync | (kLrIdle << 2) | (kLrFrag << 4) | (kLrDone << 6);
NVL_HD inline uint32_t log_read_fn(uint32_t cls) {
  return log_read_next(kLrResync, cls) | (log_read_next(kLrIdle, cls) << 2) | (log_read_next(kLrFrag, cls) << 4) |
         (log_read_next(kLrDone, cls) << 6);
}
NVL_HD inline uint32_t log_read_apply(uint32_t fn, uint32_t state) { return (fn >> (2u * state)) & 3u; }
NVL_HD inline uint32_t log_read_compose(uint32_t a, uint32_t b) {
  return log_read_apply(b, log_read_apply(a, 0u)) | (log_read_apply(b, log_read_apply(a, 1u)) << 2) |
         (log_read_apply(b, log_read_apply(a, 2u)) << 4) | (log_read_apply(b, log_read_apply(a, 3u)) << 6);
}

// What one event emits.
struct LogReadStep {
  uint32_t n_reports;     // 0 .. 2, all issued before the record, if any
  nvl_log_report rep[2];
  uint32_t record;        // 1: ReadRecord returns true here
  uint32_t joined;        // the record continues the open one (LAST): its bytes = scratch + span
};

// ReportDrop's filter (:192-197): pos_ - bytes >= initial_offset, unsigned.
NVL_HD inline bool log_read_passes(uint64_t pos, uint64_t bytes, uint64_t initial_offset) {
  return pos - bytes >= initial_offset;
}

// The event e met in `state` with `scratch` bytes collected (state kLrFrag
// only).  (Both reports have a fixed slot until the end: no indexing by a
// count, which the kernels would pay for with private memory.)
NVL_HD inline LogReadStep log_read_step(uint32_t state, uint64_t scratch, const LogReadEvent& e,
                                        uint64_t initial_offset) {
  LogReadStep s{};
  if (state == kLrDone) return s;
  const uint64_t pos = e.offset + e.span + (e.rec ? kLogHdr : 0u);  // end_of_buffer_offset_ - buffer_.size()
  // ReadPhysicalRecord's own report (:236,:264)
  const bool own = e.phys && log_read_passes(pos, e.span, initial_offset);
  uint64_t bytes = 0;
  uint32_t reason = 0;  // ReadRecord's report, if any
  if (state == kLrResync && (e.cls == kLcMiddle || e.cls == kLcLast)) {
    // swallowed (:86-95)
  } else {
    const bool frag = state == kLrFrag;  // (kLrResync: processed as from idle)
    switch (e.cls) {
      case kLcFull:  // :96-112 (an empty scratch after a FIRST: the old writer's bug, no report)
        if (frag && scratch) bytes = scratch, reason = NVL_LOG_REASON_PARTIAL_1;
        s.record = 1u;
        break;
      case kLcFirst:  // :114-129
        if (frag && scratch) bytes = scratch, reason = NVL_LOG_REASON_PARTIAL_2;
        break;
      case kLcMiddle:  // :131-138
        if (!frag) bytes = e.span, reason = NVL_LOG_REASON_MISSING_START_1;
        break;
      case kLcLast:  // :140-150
        if (!frag) bytes = e.span, reason = NVL_LOG_REASON_MISSING_START_2;
        else s.record = s.joined = 1u;
        break;
      case kLcBad:  // :161-167 (reported with 0 bytes too)
        if (frag) bytes = scratch, reason = NVL_LOG_REASON_IN_MIDDLE;
        break;
      case kLcUnknown:  // :169-178
        bytes = e.span + (frag ? scratch : 0u), reason = NVL_LOG_REASON_UNKNOWN_TYPE;
        break;
      default:  // kEof (:152-159): an open record is dropped without a report
        break;
    }
  }
  const bool mine = reason && log_read_passes(pos, bytes, initial_offset);
  const nvl_log_report r_own{e.span, e.phys, 0u};
  const nvl_log_report r_mine{bytes, reason, reason == NVL_LOG_REASON_UNKNOWN_TYPE ? (uint32_t)e.type : 0u};
  s.rep[0] = own ? r_own : r_mine;
  s.rep[1] = r_mine;
  s.n_reports = (own ? 1u : 0u) + (mine ? 1u : 0u);
  return s;
}

// SkipToInitialBlock (:36-60): the block the reader starts in.
NVL_HD inline uint64_t log_read_block_start(uint64_t initial_offset) {
  const uint64_t in_block = initial_offset % kLogBlk;
  const uint64_t start = initial_offset - in_block;
  return in_block > kLogBlk - 6u ? start + kLogBlk : start;
}

// The entry points' argument check (false: NVL_CRC32C_EINVAL); the totals are
// zero on every error return.  `query`: the three outputs are all NULL.
inline bool log_read_args(const void* data, uint64_t len, const void* payload, const void* records,
                          const void* reports, nvl_log_read_totals* totals, bool* query) {
  if (totals) *totals = nvl_log_read_totals{0, 0, 0};
  *query = !payload && !records && !reports;
  return (data || !len) && totals;
}

}  // namespace nvl
