// tests/native/log_read_asan.cc -- host-only ASan/UBSan driver of the record
// rules (nvlevelz_amd/csrc/crc32c_log_read_core.h) through nvl_log_read with
// the host CRC (tests/test_log_read.py).  Input file: cases of
//   u64 image bytes | u64 initial_offset | u64 checksum | the image
// Each is read twice -- the totals query, then with outputs of exactly the
// reported sizes on the heap, so a byte written past any of them is caught --
// and its trace (the format of tests/native/shim_harness.cc) goes to stdout,
// cases separated by a line "=".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "nvl_framing.h"

// The one device entry crc32c_framing.cpp refers to (never reached with NVL_FRAMING_HOST).
extern "C" int nvl_crc32c_batch_region_host(const void*, uint64_t, const uint64_t*, const uint64_t*, const uint32_t*,
                                            uint32_t, uint32_t*, uint64_t, uint32_t) {
  fprintf(stderr, "device path reached in a host-mode run\n");
  abort();
}

namespace nvl {
uint32_t host_extend(uint32_t init, const void* data, size_t n);  // crc32c_host.cpp
}

static const char* reason_text(const nvl_log_report& r, char* buf, size_t n) {
  static const char* const kText[] = {"",
                                      "bad record length",
                                      "checksum mismatch",
                                      "partial record without end(1)",
                                      "partial record without end(2)",
                                      "missing start of fragmented record(1)",
                                      "missing start of fragmented record(2)",
                                      "error in middle of record"};
  if (r.reason >= 1 && r.reason <= 7) return kText[r.reason];
  snprintf(buf, n, "unknown record type %u", (unsigned)r.type);
  return buf;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t head[3];
  int cases = 0;
  while (fread(head, sizeof(head), 1, f) == 1) {
    uint8_t* img = static_cast<uint8_t*>(malloc(head[0] ? head[0] : 1));  // exact size: an overread is caught
    if (head[0] && fread(img, head[0], 1, f) != 1) return 2;
    nvl_log_read_totals t, t2;
    if (nvl_log_read(img, head[0], head[1], (int)head[2], nullptr, 0, nullptr, 0, nullptr, 0, &t, NVL_FRAMING_HOST) != 0)
      return 3;
    uint8_t* payload = static_cast<uint8_t*>(malloc(t.payload_bytes ? t.payload_bytes : 1));
    nvl_log_record* rec = static_cast<nvl_log_record*>(malloc((t.n_records ? t.n_records : 1) * sizeof(nvl_log_record)));
    nvl_log_report* rep = static_cast<nvl_log_report*>(malloc((t.n_reports ? t.n_reports : 1) * sizeof(nvl_log_report)));
    if (nvl_log_read(img, head[0], head[1], (int)head[2], payload, t.payload_bytes, rec, t.n_records, rep, t.n_reports,
                     &t2, NVL_FRAMING_HOST) != 0)
      return 4;
    if (memcmp(&t, &t2, sizeof(t)) != 0) return 5;
    uint64_t r = 0;
    char buf[48];
    for (uint64_t k = 0; k <= t.n_records; ++k) {
      const uint64_t upto = k < t.n_records ? rec[k].reports_before : t.n_reports;
      for (; r < upto; ++r)
        printf("C %llu Corruption: %s\n", (unsigned long long)rep[r].bytes, reason_text(rep[r], buf, sizeof(buf)));
      if (k < t.n_records)
        printf("R %llu %llu %u\n", (unsigned long long)rec[k].offset, (unsigned long long)rec[k].length,
               nvl::host_extend(0, payload + rec[k].payload, rec[k].length));
    }
    printf("E\n=\n");
    free(rep);
    free(rec);
    free(payload);
    free(img);
    ++cases;
  }
  fclose(f);
  fprintf(stderr, "%d cases\n", cases);
  return 0;
}
