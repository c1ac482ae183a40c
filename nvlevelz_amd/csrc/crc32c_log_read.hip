// nvlevelz_amd/csrc/crc32c_log_read.hip -- the device side of nvl_log_read_dev
// (crc32c_framing_dev.cpp): the events of the device log scan
// (crc32c_log_dev.hip) become log::Reader::ReadRecord's logical records and
// corruption reports, and the records' bytes are gathered, without the image
// leaving HBM.  The record rules are crc32c_log_read_core.h's, shared with
// the host loop of nvl_log_read; here they are composed as prefix scans.
// Kernels, in stream order, ordered by kernel boundaries alone (no workgroup
// ever waits for another; every scan over the events is reduce, scan of the
// tile sums by one looped workgroup, apply, as three launches):
//
//   classify  per scan window: its nvl_log_events -> the whole image's table
//             of LogReadEvents (16 B each), kept across the windows so the
//             record pass runs once and no result depends on the window size.
//   reduce A  per tile of 1024 events: the composition of the events' state
//             maps (four states, 8 bits), the latest FIRST and the fragment
//             bytes since it (log_read_fn / log_read_compose).
//   tiles A   exclusive scan of the tile sums.
//   apply A   per event: the reader's state before it, its governing FIRST
//             and scratch->size(); then log_read_step counts what it emits
//             (records, reports, record bytes), summed per tile.
//   tiles B   exclusive scan of those; its last element is the totals.
//   emit      log_read_step again, now with every event's output places:
//             nvl_log_records (+ each record's first event), nvl_log_reports.
//   gather    one thread per aligned 16 bytes of the payload: finds its
//             record (binary search over the records' payload offsets, first
//             narrowed per workgroup) and its fragment (over the scratch
//             sizes of the record's events), then copies from offset + 7.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc32c_internal.h"
#include "crc32c_log_read_core.h"
#include "nvl_framing.h"

namespace nvl {
namespace dev {
namespace {

constexpr uint32_t kLrThreads = 256, kLrItems = 4, kLrTile = kLrThreads * kLrItems;
constexpr uint32_t kGatherChunks = 4;  // aligned 16-byte pieces per gather thread

// State map, latest FIRST (event index + 1; 0: none) and the fragment bytes
// since it (none: all the fragment bytes) of a run of events.
struct ElemA {
  uint32_t fn, first;
  uint64_t since;
};
struct OpA {
  __device__ static ElemA identity() { return ElemA{kLogReadFnId, 0u, 0u}; }
  __device__ ElemA operator()(const ElemA& a, const ElemA& b) const {  // a, then b
    return ElemA{log_read_compose(a.fn, b.fn), b.first ? b.first : a.first, b.first ? b.since : a.since + b.since};
  }
};
__device__ __forceinline__ ElemA elem_a(const LogReadEvent& e, uint32_t i) {
  return ElemA{log_read_fn(e.cls), e.cls == kLcFirst ? i + 1u : 0u, log_read_fragment_bytes(e)};
}

// What a run of events emits.
struct ElemB {
  uint32_t nrec, nrep;
  uint64_t bytes;
};
struct OpB {
  __device__ static ElemB identity() { return ElemB{0u, 0u, 0u}; }
  __device__ ElemB operator()(const ElemB& a, const ElemB& b) const {
    return ElemB{a.nrec + b.nrec, a.nrep + b.nrep, a.bytes + b.bytes};
  }
};

// Exclusive scan of one value per thread over the workgroup (kLrThreads
// threads, s: that many T in LDS); *total = all of them.  Order-preserving:
// op need not commute.
template <class T, class Op>
__device__ __forceinline__ T block_exclusive(T v, Op op, T* s, T* total) {
  const uint32_t t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kLrThreads; d <<= 1) {
    T x = Op::identity();
    if (t >= d) x = s[t - d];
    __syncthreads();
    if (t >= d) s[t] = op(x, s[t]);
    __syncthreads();
  }
  const T ex = t ? s[t - 1u] : Op::identity();
  *total = s[kLrThreads - 1u];
  __syncthreads();
  return ex;
}

// The reader's view of event i from what apply A stored.
struct Before {
  uint32_t state;
  uint64_t scratch;
};

}  // namespace

// table[i] = log_read_classify(events[i]) for the n events of a window.
__global__ __launch_bounds__(256) void crc32c_log_read_classify(const nvl_log_event* __restrict__ events, uint32_t n,
                                                                uint64_t initial_offset,
                                                                LogReadEvent* __restrict__ table) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) table[i] = log_read_classify(events[i], initial_offset);
}

// agg[tile] = the events of the tile composed.
__global__ __launch_bounds__(kLrThreads) void crc32c_log_read_reduce(const LogReadEvent* __restrict__ table, uint32_t n,
                                                                    ElemA* __restrict__ agg) {
  __shared__ ElemA s[kLrThreads];
  const uint32_t i0 = blockIdx.x * kLrTile + threadIdx.x * kLrItems;
  OpA op;
  ElemA v = OpA::identity();
  for (uint32_t k = 0; k < kLrItems; ++k)
    if (i0 + k < n) v = op(v, elem_a(table[i0 + k], i0 + k));
  ElemA total;
  (void)block_exclusive(v, op, s, &total);
  if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// out[t] = in[0] o ... o in[t - 1] for t = 0..n (out[n]: all of them), one
// workgroup looping over kLrThreads elements at a time.
template <class T, class Op>
__global__ __launch_bounds__(kLrThreads) void crc32c_log_read_tiles(const T* __restrict__ in, T* __restrict__ out,
                                                                   uint32_t n) {
  __shared__ T s[kLrThreads];
  Op op;
  T carry = Op::identity();
  for (uint32_t base = 0; base < n; base += kLrThreads) {
    const uint32_t i = base + threadIdx.x;
    T total;
    const T ex = block_exclusive(i < n ? in[i] : Op::identity(), op, s, &total);
    if (i < n) out[i] = op(carry, ex);
    carry = op(carry, total);
  }
  if (threadIdx.x == 0) out[n] = carry;
}

// Per event: state before it (state[i]), its governing FIRST (first[i], index
// + 1) and the bytes collected since that FIRST (scratch[i]); per tile: what
// its events emit (agg[tile]).  state0: the reader's state before event 0.
__global__ __launch_bounds__(kLrThreads) void crc32c_log_read_apply(const LogReadEvent* __restrict__ table, uint32_t n,
                                                                   const ElemA* __restrict__ tile_prefix,
                                                                   uint32_t state0, uint64_t initial_offset,
                                                                   uint8_t* __restrict__ state,
                                                                   uint32_t* __restrict__ first,
                                                                   uint64_t* __restrict__ scratch,
                                                                   ElemB* __restrict__ agg) {
  __shared__ ElemA sa[kLrThreads];
  __shared__ ElemB sb[kLrThreads];
  const uint32_t i0 = blockIdx.x * kLrTile + threadIdx.x * kLrItems;
  OpA op;
  LogReadEvent e[kLrItems];
  ElemA v = OpA::identity();
#pragma unroll
  for (uint32_t k = 0; k < kLrItems; ++k)
    if (i0 + k < n) {
      e[k] = table[i0 + k];
      v = op(v, elem_a(e[k], i0 + k));
    }
  ElemA total;
  ElemA cur = op(tile_prefix[blockIdx.x], block_exclusive(v, op, sa, &total));
  OpB opb;
  ElemB b = OpB::identity();
#pragma unroll
  for (uint32_t k = 0; k < kLrItems; ++k)
    if (i0 + k < n) {
      const uint32_t st = log_read_apply(cur.fn, state0);
      state[i0 + k] = (uint8_t)st;
      first[i0 + k] = cur.first;
      scratch[i0 + k] = cur.since;
      const LogReadStep s = log_read_step(st, cur.since, e[k], initial_offset);
      b = opb(b, ElemB{s.record, s.n_reports, s.record ? (s.joined ? cur.since : 0u) + e[k].span : 0u});
      cur = op(cur, elem_a(e[k], i0 + k));
    }
  ElemB tb;
  (void)block_exclusive(b, opb, sb, &tb);
  if (threadIdx.x == 0) agg[blockIdx.x] = tb;
}

// The records (with each one's first event in rec_first) and the reports, at
// the places the scan of the counts gives them.
__global__ __launch_bounds__(kLrThreads) void crc32c_log_read_emit(const LogReadEvent* __restrict__ table, uint32_t n,
                                                                  const ElemB* __restrict__ tile_prefix,
                                                                  uint64_t initial_offset,
                                                                  const uint8_t* __restrict__ state,
                                                                  const uint32_t* __restrict__ first,
                                                                  const uint64_t* __restrict__ scratch,
                                                                  nvl_log_record* __restrict__ records,
                                                                  uint32_t* __restrict__ rec_first,
                                                                  nvl_log_report* __restrict__ reports) {
  __shared__ ElemB sb[kLrThreads];
  const uint32_t i0 = blockIdx.x * kLrTile + threadIdx.x * kLrItems;
  OpB opb;
  ElemB b = OpB::identity();
#pragma unroll
  for (uint32_t k = 0; k < kLrItems; ++k)
    if (i0 + k < n) {
      const LogReadEvent e = table[i0 + k];
      const LogReadStep s = log_read_step(state[i0 + k], scratch[i0 + k], e, initial_offset);
      b = opb(b, ElemB{s.record, s.n_reports, s.record ? (s.joined ? scratch[i0 + k] : 0u) + e.span : 0u});
    }
  ElemB tb;
  ElemB cur = opb(tile_prefix[blockIdx.x], block_exclusive(b, opb, sb, &tb));
#pragma unroll
  for (uint32_t k = 0; k < kLrItems; ++k)
    if (i0 + k < n) {
      const uint32_t i = i0 + k;
      const LogReadEvent e = table[i];
      const LogReadStep s = log_read_step(state[i], scratch[i], e, initial_offset);
      if (s.n_reports > 0u) reports[cur.nrep] = s.rep[0];
      if (s.n_reports > 1u) reports[cur.nrep + 1u] = s.rep[1];
      cur.nrep += s.n_reports;
      if (s.record) {
        const uint32_t f0 = s.joined ? first[i] - 1u : i;
        const uint64_t length = (s.joined ? scratch[i] : 0u) + e.span;
        records[cur.nrec] = nvl_log_record{table[f0].offset, cur.bytes, length, i - f0 + 1u, cur.nrep};
        rec_first[cur.nrec] = f0;
        ++cur.nrec;
        cur.bytes += length;
      }
    }
}

namespace {

// The last k in [lo, hi] with records[k].payload <= d (lo's is).
__device__ __forceinline__ uint32_t find_record(const nvl_log_record* __restrict__ records, uint32_t lo, uint32_t hi,
                                                uint64_t d) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1u) / 2u;
    if (records[mid].payload <= d) lo = mid;
    else hi = mid - 1u;
  }
  return lo;
}

// A record's fragments are the events [j, j + fragments); fragment f starts
// at scratch[f] bytes into the record (j: at 0).
struct Frag {
  uint32_t f, last;      // the event, the record's last event
  uint64_t start, end;   // its bytes in the record: [start, end)
  uint64_t src;          // image offset of its first byte
};
__device__ __forceinline__ Frag frag_at(const LogReadEvent* __restrict__ table, const uint64_t* __restrict__ scratch,
                                        uint32_t j, uint32_t f, uint32_t last) {
  const LogReadEvent e = table[f];
  const uint64_t start = f == j ? 0u : scratch[f];
  return Frag{f, last, start, start + e.span, e.offset + kLogHdr};
}
// The fragment of record (j, fragments) holding byte x of it (x < its length).
__device__ __forceinline__ Frag find_frag(const LogReadEvent* __restrict__ table, const uint64_t* __restrict__ scratch,
                                          uint32_t j, uint32_t fragments, uint64_t x) {
  uint32_t lo = j, hi = j + fragments - 1u;
  const uint32_t last = hi;
  while (lo < hi) {  // the last f with start(f) <= x
    const uint32_t mid = lo + (hi - lo + 1u) / 2u;
    if (scratch[mid] <= x) lo = mid;
    else hi = mid - 1u;
  }
  return frag_at(table, scratch, j, lo, last);
}

}  // namespace

// payload[0, total) = the records' bytes.  Chunk c is the aligned 16 bytes at
// (payload & ~15) + 16 c; a workgroup takes kLrThreads * kGatherChunks
// consecutive chunks, chunk by chunk across its threads.  The image is read
// inside [data, data + len) only, the payload written inside [0, total) only.
__global__ __launch_bounds__(kLrThreads) void crc32c_log_read_gather(const uint8_t* __restrict__ data, uint64_t len,
                                                                    const LogReadEvent* __restrict__ table,
                                                                    const uint64_t* __restrict__ scratch,
                                                                    const nvl_log_record* __restrict__ records,
                                                                    const uint32_t* __restrict__ rec_first,
                                                                    uint32_t nrec, uint8_t* __restrict__ payload,
                                                                    uint64_t total) {
  __shared__ uint32_t s_k[2];
  const uint64_t a = (uint64_t)((uintptr_t)payload & 15u);
  const uint64_t c0 = (uint64_t)blockIdx.x * (kLrThreads * kGatherChunks);
  // the records of the workgroup's first and last byte: every thread's search stays between them
  if (threadIdx.x == 0 || threadIdx.x == 64) {
    const uint64_t lo = c0 * 16u > a ? c0 * 16u - a : 0u;
    uint64_t hi = (c0 + kLrThreads * kGatherChunks) * 16u - a;  // (> 0: a < 16)
    hi = hi < total ? hi : total;
    const uint64_t d = threadIdx.x == 0 ? lo : hi - 1u;
    s_k[threadIdx.x ? 1 : 0] = lo < hi ? find_record(records, 0u, nrec - 1u, d) : 0u;
  }
  __syncthreads();
  const uint32_t klo = s_k[0], khi = s_k[1];
  const uintptr_t img_lo = (uintptr_t)data, img_hi = (uintptr_t)data + len;
  for (uint32_t q = 0; q < kGatherChunks; ++q) {
    const uint64_t c = c0 + (uint64_t)q * kLrThreads + threadIdx.x;
    const uint64_t d0 = c * 16u > a ? c * 16u - a : 0u;
    uint64_t d1 = (c + 1u) * 16u - a;
    d1 = d1 < total ? d1 : total;
    if (d0 >= d1) continue;
    uint32_t k = find_record(records, klo, khi, d0);
    nvl_log_record rec = records[k];
    uint32_t j = rec_first[k];
    uint64_t x = d0 - rec.payload;  // the byte's place in its record
    Frag fr = rec.fragments == 1u ? frag_at(table, scratch, j, j, j) : find_frag(table, scratch, j, rec.fragments, x);
    uint8_t* out = payload + d0;
    if (d1 - d0 == 16u && x + 16u <= fr.end) {  // a whole aligned piece from one fragment
      const uint8_t* src = data + fr.src + (x - fr.start);
      const uintptr_t sp = (uintptr_t)src;
      uint4 v;
      if ((sp & 15u) == 0u) {
        v = *reinterpret_cast<const uint4*>(src);
      } else if ((sp & 3u) == 0u) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(src);
        v = make_uint4(w[0], w[1], w[2], w[3]);
      } else if ((sp & ~(uintptr_t)3u) >= img_lo && (sp & ~(uintptr_t)3u) + 20u <= img_hi) {
        // five aligned words around the piece, shifted into place
        const uint32_t* w = reinterpret_cast<const uint32_t*>(sp & ~(uintptr_t)3u);
        const uint32_t sh = 8u * (uint32_t)(sp & 3u), w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
        v = make_uint4((w0 >> sh) | (w1 << (32u - sh)), (w1 >> sh) | (w2 << (32u - sh)),
                       (w2 >> sh) | (w3 << (32u - sh)), (w3 >> sh) | (w4 << (32u - sh)));
      } else {  // (the image's own first or last bytes)
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t i = 0; i < 16u; ++i) w[i >> 2] |= (uint32_t)src[i] << (8u * (i & 3u));
        v = make_uint4(w[0], w[1], w[2], w[3]);
      }
      *reinterpret_cast<uint4*>(out) = v;
      continue;
    }
    // the payload's first or last bytes, or a piece over a fragment seam: byte by byte
    for (uint64_t d = d0; d < d1; ++d, ++x) {
      while (x >= fr.end) {  // (ends: byte d < total lies in some fragment; empty ones are passed over)
        if (fr.f < fr.last) {
          fr = frag_at(table, scratch, j, fr.f + 1u, fr.last);
        } else {
          rec = records[++k];
          j = rec_first[k];
          x = d - rec.payload;
          fr = frag_at(table, scratch, j, j, j + rec.fragments - 1u);
        }
      }
      payload[d] = data[fr.src + (x - fr.start)];
    }
  }
}

}  // namespace dev

hipError_t launch_log_read_classify(const nvl_log_event* events, uint32_t n, uint64_t initial_offset,
                                    LogReadEvent* table, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::crc32c_log_read_classify, dim3((n + 255u) / 256u), dim3(256), 0, st, events, n,
                     initial_offset, table);
  return hipGetLastError();
}

uint32_t log_read_tiles(uint32_t n) { return (n + dev::kLrTile - 1u) / dev::kLrTile; }

hipError_t launch_log_read_count(const LogReadEvent* table, uint32_t n, uint32_t state0, uint64_t initial_offset,
                                 void* tiles_a, void* tiles_b, uint8_t* state, uint32_t* first, uint64_t* scratch,
                                 hipStream_t st) {
  const uint32_t nt = log_read_tiles(n);
  // tiles_a: [nt sums][nt + 1 prefixes] of 16 bytes; tiles_b the same
  dev::ElemA* agg_a = static_cast<dev::ElemA*>(tiles_a);
  dev::ElemB* agg_b = static_cast<dev::ElemB*>(tiles_b);
  hipLaunchKernelGGL(dev::crc32c_log_read_reduce, dim3(nt), dim3(dev::kLrThreads), 0, st, table, n, agg_a);
  hipLaunchKernelGGL((dev::crc32c_log_read_tiles<dev::ElemA, dev::OpA>), dim3(1), dim3(dev::kLrThreads), 0, st,
                     static_cast<const dev::ElemA*>(agg_a), agg_a + nt, nt);
  hipLaunchKernelGGL(dev::crc32c_log_read_apply, dim3(nt), dim3(dev::kLrThreads), 0, st, table, n,
                     static_cast<const dev::ElemA*>(agg_a + nt), state0, initial_offset, state, first, scratch, agg_b);
  hipLaunchKernelGGL((dev::crc32c_log_read_tiles<dev::ElemB, dev::OpB>), dim3(1), dim3(dev::kLrThreads), 0, st,
                     static_cast<const dev::ElemB*>(agg_b), agg_b + nt, nt);
  return hipGetLastError();
}

hipError_t launch_log_read_emit(const LogReadEvent* table, uint32_t n, uint64_t initial_offset, const void* tiles_b,
                                const uint8_t* state, const uint32_t* first, const uint64_t* scratch,
                                nvl_log_record* records, uint32_t* rec_first, nvl_log_report* reports,
                                hipStream_t st) {
  const uint32_t nt = log_read_tiles(n);
  hipLaunchKernelGGL(dev::crc32c_log_read_emit, dim3(nt), dim3(dev::kLrThreads), 0, st, table, n,
                     static_cast<const dev::ElemB*>(tiles_b) + nt, initial_offset, state, first, scratch, records,
                     rec_first, reports);
  return hipGetLastError();
}

hipError_t launch_log_read_gather(const void* data, uint64_t len, const LogReadEvent* table, const uint64_t* scratch,
                                  const nvl_log_record* records, const uint32_t* rec_first, uint32_t nrec,
                                  void* payload, uint64_t total, hipStream_t st) {
  if (total == 0 || nrec == 0) return hipSuccess;
  const uint64_t chunks = (((uintptr_t)payload & 15u) + total + 15u) / 16u;
  const uint64_t per = (uint64_t)dev::kLrThreads * dev::kGatherChunks;
  const uint64_t grid = (chunks + per - 1u) / per;
  if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dev::crc32c_log_read_gather, dim3((uint32_t)grid), dim3(dev::kLrThreads), 0, st,
                     static_cast<const uint8_t*>(data), len, table, scratch, records, rec_first, nrec,
                     static_cast<uint8_t*>(payload), total);
  return hipGetLastError();
}

}  // namespace nvl
