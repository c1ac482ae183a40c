#!/usr/bin/env python3
"""Record tests/golden/log_read_cases.json: the REFERENCE's log::Reader trace
(ref_log_read of oracle/_ref/libref_framing.so, built by oracle/reftests.mk)
of every record-level edge image of tests/log_read_cases.py.  The file holds
data only: each case's name, initial_offset, checksum flag, the image's
length and CRC32C (the images are rebuilt from their seeds by the tests and
checked against these) and the trace.

    python tools/gen_log_read_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import oracle  # noqa: E402
import log_read_cases as lrc  # noqa: E402


def main():
    rf = oracle.ref_framing()
    port = oracle.port()
    cases = []
    for name, img, initial_offset, checksum in lrc.edge_cases():
        cases.append({"name": name, "initial_offset": initial_offset, "checksum": bool(checksum),
                      "image_len": len(img), "image_crc": port.value(img),
                      "trace": rf.log_read(img, bool(checksum), initial_offset)})
    out = {"provenance": "tools/gen_log_read_golden.py: ref_log_read (the reference's db/log_reader.cc) over "
                         "tests/log_read_cases.py:edge_cases()", "cases": cases}
    path = os.path.join(ROOT, "tests", "golden", "log_read_cases.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(len(cases), "cases ->", path)


if __name__ == "__main__":
    main()
