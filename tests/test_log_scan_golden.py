"""nvl_log_scan(..., NVL_FRAMING_HOST) against recorded events: the host scan
and the log kernels run the same block rules (nvlevelz_amd/csrc/
crc32c_log_core.h), so tests/test_log_scan_dev.py's device-versus-host
identity cannot see a rule bug that both sides share.  This module pins the
host side on the same images: tests/golden/log_scan_events.json holds the
event count and the SHA-256 of the event bytes (every field, `reserved`
included) of

* every image of edge_images() at start = 0, checksum 1 and 0;
* fuzz_image(seed) for seeds 0..199 at start 0 and 3 * 32768, checksum 1 and 0,

recorded from the scan as it stood before the rules were shared (three
separate copies: host passes, kernels, tests).  No GPU.

Record again (only when nvl_log_scan's contract changes on purpose):
`python tests/test_log_scan_golden.py`.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_log_scan_dev import BLK, KINDS, _lib, edge_images, fuzz_image, host_scan  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "log_scan_events.json")
# the events of the fixture by kind, counted when it was recorded
KIND_COUNTS = {"RECORD": 17404, "BAD_LENGTH": 296, "CHECKSUM": 136, "ZERO": 270, "EOF": 854}


def cases():
    """(name, image, start, checksum) of the 854 cases, in the fixture's order."""
    for name, img in edge_images():
        for checksum in (1, 0):
            yield f"edge/{name}/c{checksum}", img, 0, checksum
    for seed in range(200):
        img = fuzz_image(seed)
        for start in (0, 3 * BLK):
            for checksum in (1, 0):
                yield f"fuzz/{seed}/s{start}/c{checksum}", img, start, checksum


def scan_all():
    """({name: [count, sha256 of the events]}, events per kind)."""
    L = _lib()
    out = {}
    kinds = np.zeros(len(KINDS), dtype=np.int64)
    for name, img, start, checksum in cases():
        n, raw = host_scan(L, img, start, checksum)
        assert len(raw) == 32 * n, name
        out[name] = [n, hashlib.sha256(raw).hexdigest()]
        kinds += np.bincount(np.frombuffer(raw, dtype="<u4").reshape(-1, 8)[:, 6], minlength=len(KINDS))
    return out, dict(zip(KINDS, (int(k) for k in kinds)))


def test_host_scan_matches_the_recorded_events():
    with open(FIXTURE) as f:
        want = json.load(f)
    got, kinds = scan_all()
    assert len(got) == 854 and sorted(got) == sorted(want["cases"])
    bad = [(k, got[k], want["cases"][k]) for k in got if got[k] != want["cases"][k]]
    assert not bad, (len(bad), bad[:5])
    # the fixture holds every kind of event
    assert want["kinds"] == KIND_COUNTS
    assert kinds == KIND_COUNTS


if __name__ == "__main__":
    got, kinds = scan_all()
    assert len(got) == 854, len(got)
    with open(FIXTURE, "w") as f:
        json.dump({"kinds": kinds, "cases": got}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", len(got), "cases,", kinds)
