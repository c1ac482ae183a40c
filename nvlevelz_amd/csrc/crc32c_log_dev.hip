// nvlevelz_amd/csrc/crc32c_log_dev.hip -- the device side of nvl_log_scan_dev
// / nvl_log_scan_staged (crc32c_framing_dev.cpp): a log image in HBM is
// parsed, checked and replayed on the GPU, so only the nvl_log_events return.
// The three passes of nvl_log_scan (crc32c_framing.cpp) as kernels: the block
// rules are crc32c_log_core.h's, shared with the host scan; here are the
// thread-parallel loops and the staging, ordered by kernel boundaries alone
// (no workgroup ever waits for another):
//
//   parse    one wave per 32 KiB log block (log::Reader restarts its parse at
//            every block, db/log_reader.cc:199-218): the block is staged into
//            LDS with 16-byte loads and one lane walks the record headers
//            there (log_walk_block) -- a hop in LDS instead of a dependent
//            HBM miss per record.  Per block: a LogBlockInfo and every
//            candidate's position in the block (u16).
//   scan     exclusive prefix sum of the per-block counts (one looped
//            workgroup: there is one element per 32 KiB of log).
//   expand   the candidates in file order as the offsets[] / lengths[] of
//            nvl_crc32c_region_dev (log_slot).
//   (CRC)    nvl_crc32c_region_dev over the image, NVL_CRC32C_FLAG_REGION_SHAPED:
//            the candidates are sorted, disjoint, at most 32762 bytes and
//            inside the image by construction.
//   verdict  every candidate checks its CRC (log_crc_ok); a block is cut at
//            its first mismatch and counts the events it emits.
//   scan     the emitted counts to bases.
//   emit     the events in reader order.
//
// Workspace per window of nblk blocks holding n candidates (the formula of
// crc32c_framing_dev.cpp's log_ws): nblk * (16 + 5 * 4) + 5 * 4 bytes of
// per-block words, the position slab of nblk * 4682 * 2 bytes (28.6 % of the
// image bytes), and per candidate 8 + 8 + 4 bytes (offsets, lengths, CRCs)
// plus the region workspace and 32 bytes per event returned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc32c_internal.h"
#include "crc32c_log_core.h"
#include "nvl_framing.h"

namespace nvl {
namespace dev {
namespace {

constexpr uint32_t kScanThreads = 1024;

// One 16-byte piece of the image at g, bytes outside [lo, hi) read as zero
// and never touched (the first piece of the image when its pointer is not
// 16-byte aligned, the last one when its end is not).
__device__ __forceinline__ uint4 load_edge16(const uint8_t* g, const uint8_t* lo, const uint8_t* hi) {
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) {
    const uint8_t* q = g + i;
    const uint32_t b = ((uintptr_t)q >= (uintptr_t)lo && (uintptr_t)q < (uintptr_t)hi) ? (uint32_t)*q : 0u;
    w[i >> 2] |= b << (8u * (i & 3u));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace

// Block blockIdx.x of the image [data, data + len): bytes [b0, b0 + m), m =
// min(32768, len - b0); a short block (m < 32768, the last one) is where the
// input ends.  LDS byte a + i holds block byte i, a = the block's misalignment
// to 16 bytes, so every global load is an aligned 16-byte one.
__global__ __launch_bounds__(64) void crc32c_log_parse(const uint8_t* __restrict__ data, uint64_t len,
                                                       uint16_t* __restrict__ slab, LogBlockInfo* __restrict__ info,
                                                       uint32_t* __restrict__ cnt) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kLogBlk + 16u];
  const uint32_t blk = blockIdx.x, lane = threadIdx.x;
  const uint64_t b0 = (uint64_t)blk * kLogBlk;
  const uint64_t rem = len - b0;  // (b0 <= len: the launcher's grid is len / 32768 + 1 blocks at most)
  const uint32_t m = rem < kLogBlk ? (uint32_t)rem : kLogBlk;
  const uint8_t* p = data + b0;
  const uint32_t a = (uint32_t)((uintptr_t)p & 15u);
  const uint8_t* pa = p - a;
  const uint32_t nv = m ? (a + m + 15u) / 16u : 0u;
  const uint8_t* hi = data + len;
  for (uint32_t j = lane; j < nv; j += 64u) {
    const uint8_t* g = pa + 16u * j;
    uint4 v;
    if ((uintptr_t)g >= (uintptr_t)data && (uintptr_t)g + 16u <= (uintptr_t)hi) v = *reinterpret_cast<const uint4*>(g);
    else v = load_edge16(g, data, hi);
    *reinterpret_cast<uint4*>(lds + 16u * j) = v;
  }
  __syncthreads();
  if (lane != 0) return;
  // one lane walks the headers in LDS; the block's kLogSlab positions hold any block's candidates
  const LogBlockInfo bi = log_walk_block(lds + a, m, slab + (uint64_t)blk * kLogSlab);
  info[blk] = bi;
  cnt[blk] = bi.count;
}

// out[i] = in[0] + ... + in[i - 1] for i = 0..n (out[n]: the total), one
// workgroup looping over 1024 elements at a time.
__global__ __launch_bounds__(kScanThreads) void crc32c_log_scan(const uint32_t* __restrict__ in,
                                                                uint32_t* __restrict__ out, uint32_t n) {
  __shared__ uint32_t s[kScanThreads];
  const uint32_t t = threadIdx.x;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n; base += kScanThreads) {
    const uint32_t i = base + t;
    const uint32_t v = i < n ? in[i] : 0u;
    s[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
      const uint32_t x = t >= d ? s[t - d] : 0u;
      __syncthreads();
      s[t] += x;
      __syncthreads();
    }
    if (i < n) out[i] = carry + s[t] - v;
    carry += s[kScanThreads - 1u];
    __syncthreads();
  }
  if (t == 0) out[n] = carry;
}

// Candidate k of block blockIdx.x -> batch slot base[blk] + k.
__global__ __launch_bounds__(256) void crc32c_log_expand(const uint16_t* __restrict__ slab,
                                                         const LogBlockInfo* __restrict__ info,
                                                         const uint32_t* __restrict__ base,
                                                         uint64_t* __restrict__ off, uint64_t* __restrict__ ln) {
  const uint32_t blk = blockIdx.x;
  const LogBlockInfo bi = info[blk];
  const uint16_t* s = slab + (uint64_t)blk * kLogSlab;
  const uint64_t b0 = (uint64_t)blk * kLogBlk, k0 = base[blk];
  for (uint32_t k = threadIdx.x; k < bi.count; k += blockDim.x) {
    const LogSlot c = log_slot(bi, s, k);
    off[k0 + k] = b0 + c.off;
    ln[k0 + k] = c.len;
  }
}

// cut[blk] = the block's first candidate whose CRC does not match its header
// (count: none; nothing is compared when checksum = 0), nemit[blk] = the
// events the block emits.
__global__ __launch_bounds__(256) void crc32c_log_verdict(const uint8_t* __restrict__ data,
                                                          const uint16_t* __restrict__ slab,
                                                          const LogBlockInfo* __restrict__ info,
                                                          const uint32_t* __restrict__ base,
                                                          const uint32_t* __restrict__ crc, int checksum,
                                                          uint32_t* __restrict__ cut, uint32_t* __restrict__ nemit) {
  __shared__ uint32_t s_cut;
  const uint32_t blk = blockIdx.x;
  const LogBlockInfo bi = info[blk];
  const uint16_t* s = slab + (uint64_t)blk * kLogSlab;
  if (threadIdx.x == 0) s_cut = bi.count;
  __syncthreads();
  if (checksum) {
    const uint8_t* b = data + (uint64_t)blk * kLogBlk;
    const uint64_t k0 = base[blk];
    for (uint32_t k = threadIdx.x; k < bi.count; k += blockDim.x)
      if (!log_crc_ok(b, s, k, crc[k0 + k])) atomicMin(&s_cut, k);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  cut[blk] = s_cut;
  nemit[blk] = log_emit_count(bi, s, s_cut);
}

// The events of block blockIdx.x at events[ebase[blk] ...), those below evcap
// only; `start` is the file offset of data[0].
__global__ __launch_bounds__(256) void crc32c_log_emit(const uint8_t* __restrict__ data, uint64_t start,
                                                       const uint16_t* __restrict__ slab,
                                                       const LogBlockInfo* __restrict__ info,
                                                       const uint32_t* __restrict__ cut,
                                                       const uint32_t* __restrict__ ebase,
                                                       nvl_log_event* __restrict__ events, uint64_t evcap) {
  const uint32_t blk = blockIdx.x;
  const LogBlockInfo bi = info[blk];
  const uint16_t* s = slab + (uint64_t)blk * kLogSlab;
  const uint64_t b0 = (uint64_t)blk * kLogBlk, f0 = start + b0;
  const uint32_t c = cut[blk];
  const uint32_t nrec = c < bi.count ? c : bi.count;
  const uint64_t e0 = ebase[blk];
  for (uint32_t k = threadIdx.x; k < nrec; k += blockDim.x) {
    if (e0 + k >= evcap) break;
    events[e0 + k] = log_record_event(bi, s, k, data + b0, f0);
  }
  if (threadIdx.x != 0) return;
  uint64_t e = e0 + nrec;
  log_tail_events(bi, s, c, f0, [&](const nvl_log_event& x) {
    if (e < evcap) events[e] = x;
    ++e;
  });
}

}  // namespace dev

hipError_t launch_log_parse(const void* data, uint64_t len, uint32_t nblk, uint16_t* slab, LogBlockInfo* info,
                            uint32_t* cnt, hipStream_t st) {
  if (nblk == 0 || (uint64_t)(nblk - 1u) * NVL_LOG_BLOCK_SIZE > len) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dev::crc32c_log_parse, dim3(nblk), dim3(64), 0, st, static_cast<const uint8_t*>(data), len, slab,
                     info, cnt);
  return hipGetLastError();
}

hipError_t launch_log_scan(const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t st) {
  hipLaunchKernelGGL(dev::crc32c_log_scan, dim3(1), dim3(dev::kScanThreads), 0, st, in, out, n);
  return hipGetLastError();
}

hipError_t launch_log_expand(const uint16_t* slab, const LogBlockInfo* info, const uint32_t* base, uint32_t nblk,
                             uint64_t* off, uint64_t* len1, hipStream_t st) {
  hipLaunchKernelGGL(dev::crc32c_log_expand, dim3(nblk), dim3(256), 0, st, slab, info, base, off, len1);
  return hipGetLastError();
}

hipError_t launch_log_verdict(const void* data, const uint16_t* slab, const LogBlockInfo* info,
                              const uint32_t* base, const uint32_t* crc, int checksum, uint32_t nblk, uint32_t* cut,
                              uint32_t* nemit, hipStream_t st) {
  hipLaunchKernelGGL(dev::crc32c_log_verdict, dim3(nblk), dim3(256), 0, st, static_cast<const uint8_t*>(data), slab,
                     info, base, crc, checksum, cut, nemit);
  return hipGetLastError();
}

hipError_t launch_log_emit(const void* data, uint64_t start, const uint16_t* slab, const LogBlockInfo* info,
                           const uint32_t* cut, const uint32_t* ebase, uint32_t nblk, nvl_log_event* events,
                           uint64_t evcap, hipStream_t st) {
  hipLaunchKernelGGL(dev::crc32c_log_emit, dim3(nblk), dim3(256), 0, st, static_cast<const uint8_t*>(data), start, slab,
                     info, cut, ebase, events, evcap);
  return hipGetLastError();
}

}  // namespace nvl
