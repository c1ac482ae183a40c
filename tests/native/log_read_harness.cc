// tests/native/log_read_harness.cc -- extern "C" driver of
// nvl::shims::DeviceLogReader (include/nvl_leveldb_shims.h) for
// tests/test_log_read_dev.py: the trace format of shim_harness.cc's
// shim_log_read (and of oracle/ref_framing.cc), so the traces compare line
// for line with the reference's.  Test code, not product.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "nvl_leveldb_shims.h"

namespace {

struct TraceReporter : nvl::shims::LogReader::Reporter {
  std::string* trace;
  void Corruption(size_t bytes, const char* reason) override {
    char buf[64];
    snprintf(buf, sizeof(buf), "C %zu Corruption: ", bytes);
    trace->append(buf);
    trace->append(reason);
    trace->push_back('\n');
  }
};

}  // namespace

extern "C" {

// DeviceLogReader over a log image in device memory, on `stream`.
__attribute__((visibility("default")))
int shim_log_read_device(const void* dev_image, size_t len, int checksum, uint64_t initial_offset, void* stream,
                         char* trace, size_t cap, size_t* trace_len) {
  std::string t;
  TraceReporter rep;
  rep.trace = &t;
  nvl::shims::DeviceLogReader r(dev_image, len, stream, &rep, checksum != 0, initial_offset);
  const char* d;
  size_t n;
  std::string scratch;
  while (r.ReadRecord(&d, &n, &scratch)) {
    char buf[96];
    snprintf(buf, sizeof(buf), "R %llu %zu %u\n", (unsigned long long)r.LastRecordOffset(), n, nvl_crc32c_value(d, n));
    t.append(buf);
  }
  if (r.status() != NVL_CRC32C_OK) return r.status();
  t.append("E\n");
  *trace_len = t.size();
  if (t.size() > cap) return NVL_CRC32C_ENOSPC;
  memcpy(trace, t.data(), t.size());
  return NVL_CRC32C_OK;
}

// What a caller without the device reader does with a host copy of the
// image: a ReadRecord loop over shims::LogReader, records and their bytes
// counted (tools/shim_latency.py --log-read times it).
__attribute__((visibility("default")))
int shim_log_read_count(const uint8_t* file, size_t len, int checksum, uint64_t initial_offset, uint32_t flags,
                        uint64_t* records, uint64_t* bytes) {
  nvl::shims::LogReader r(reinterpret_cast<const char*>(file), len, nullptr, checksum != 0, initial_offset, flags);
  const char* d;
  size_t n;
  std::string scratch;
  *records = *bytes = 0;
  while (r.ReadRecord(&d, &n, &scratch)) {
    ++*records;
    *bytes += n;
  }
  return r.status();
}

}  // extern "C"
