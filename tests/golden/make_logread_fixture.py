"""Hand-framed log images the WAL fixture (make_log_fixture.py) lacks, read by
the REFERENCE's own log::Reader (common/log_reader.cc, compiled in place into
oracle/_ref/libref_log.so by `make -C oracle reflog`).

    python tests/golden/make_logread_fixture.py

Stored (tests/golden/logread_fixture.json), no image bytes: for each scenario
the framing ops and byte edits that logreadmodel.frame_image turns into the
image (payload bytes: printable_bytes(seed, ...), tests/golden/splitmix.py), and
for each initial_offset the reference reader's exact output, every ReadRecord
result and Reporter::Corruption call in order.

The scenarios: an empty image; 3 bytes; the old writer's empty FIRST in a
block's last 7 bytes followed by FULL, by FIRST and by MIDDLE + LAST; a
five-block record with its third block zeroed; a block of 4,681 empty records
and a 1-byte trailer; FIRST FIRST LAST; FIRST FULL; type 5 inside a fragmented
record; LAST and MIDDLE without a FIRST; a bad length in the short last block;
a file of exactly one block; checksum failures in two adjacent blocks of one
record; and each one that spans a block again from initial offsets inside the
span.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from logreadmodel import BLOCK, frame_image  # noqa: E402
from splitmix import printable_bytes  # noqa: E402

LIB = os.path.join(REPO, "oracle", "_ref", "libref_log.so")
SEED = 0x10C2EAD
PAY = BLOCK - 7
FULL, FIRST, MIDDLE, LAST = 1, 2, 3, 4
SPAN = [BLOCK - 8, BLOCK - 7, BLOCK - 6, BLOCK - 5, BLOCK - 1, BLOCK, BLOCK + 1, BLOCK + 7, 2 * BLOCK - 3,
        2 * BLOCK + 100, 3 * BLOCK, 4 * BLOCK + 7, 4 * BLOCK + 8]

SCENARIOS = [
    ("empty", [], [], []),
    ("three_bytes", [["z", 3]], [], [1, 3, 4]),
    ("quirk_full", [["p", FULL, PAY - 7], ["p", FIRST, 0], ["p", FULL, 5]], [], SPAN[:8]),
    ("quirk_middle_last", [["p", FULL, PAY - 7], ["p", FIRST, 0], ["p", MIDDLE, 2], ["p", LAST, 3]], [], SPAN[:8]),
    ("quirk_first", [["p", FULL, PAY - 7], ["p", FIRST, 0], ["p", FIRST, 4], ["p", LAST, 3]], [], SPAN[:8]),
    ("five_blocks_third_zeroed",
     [["p", FIRST, PAY], ["p", MIDDLE, PAY], ["p", MIDDLE, PAY], ["p", MIDDLE, PAY], ["p", LAST, 10]],
     [["zero", 2 * BLOCK, BLOCK]], SPAN),
    ("five_blocks_clean",
     [["p", FIRST, PAY], ["p", MIDDLE, PAY], ["p", MIDDLE, PAY], ["p", MIDDLE, PAY], ["p", LAST, 10], ["p", FULL, 3]],
     [], SPAN),
    ("block_of_empty_records", [["x", 4681, ["p", FULL, 0]], ["z", 1], ["p", FULL, 9]], [], SPAN[:8] + [7, 14 * 2000]),
    ("first_first_last", [["p", FIRST, 10], ["p", FIRST, 5], ["p", LAST, 3]], [], [1, 17]),
    ("first_full", [["p", FIRST, 10], ["p", FULL, 4], ["p", FULL, 2]], [], [17]),
    ("type_5_in_fragmented", [["p", FIRST, 10], ["p", 5, 3], ["p", FULL, 4]], [], [1, 17]),
    ("type_5_after_empty_first", [["p", FIRST, 0], ["p", 5, 3], ["p", FULL, 4]], [], []),
    ("last_and_middle_without_first", [["p", LAST, 4], ["p", MIDDLE, 5], ["p", FULL, 1]], [], [11, 12]),
    ("bad_length_in_short_last_block", [["p", FULL, 10], ["p", FULL, 500, 20]], [], [17, 18]),
    ("bad_length_in_fragmented", [["p", FIRST, 10], ["p", MIDDLE, 500, 20]], [], []),
    ("truncated_in_fragmented", [["p", FIRST, 10], ["z", 4]], [], [17, 18]),
    ("exactly_one_block", [["p", FULL, PAY]], [], [1, BLOCK - 6, BLOCK - 5, BLOCK]),
    ("one_block_with_trailer", [["p", FULL, PAY - 3], ["z", 3]], [], []),
    ("checksum_in_two_adjacent_blocks",
     [["p", FIRST, PAY], ["p", MIDDLE, PAY], ["p", MIDDLE, PAY], ["p", LAST, 100], ["p", FULL, 7]],
     [["xor", BLOCK + 1000, 0x20], ["xor", 2 * BLOCK + 9, 0x01]], SPAN[:11]),
    ("checksum_then_records_in_block",
     [["p", FULL, 100], ["p", FULL, 50], ["p", FULL, 60], ["p", FIRST, PAY - 3 * 7 - 210], ["p", LAST, 30],
      ["p", FULL, 8]], [["xor", 107 + 7 + 3, 0x80]], [108, BLOCK]),
    ("unknown_type_in_fragmented", [["p", FIRST, 10], ["p", 0x85, 6], ["p", 0, 3], ["p", LAST, 2]], [], [18]),
    ("zero_header_in_fragmented", [["p", FIRST, 10], ["z", 40]], [], []),
    ("empty_fragmented_record", [["p", FIRST, 0], ["p", LAST, 0], ["p", FIRST, 0], ["p", MIDDLE, 0], ["p", LAST, 1]],
     [], [7]),
]


def main():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(REPO, "oracle"), "reflog"], check=True)
    ref = ctypes.CDLL(LIB)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    ref.ref_log_read_from.restype = sz
    ref.ref_log_read_from.argtypes = [vp, sz, ctypes.c_uint64, vp, sz]
    ref.ref_log_value.restype = ctypes.c_uint32
    ref.ref_log_value.argtypes = [ctypes.c_char_p, sz]

    def value(data):
        return int(ref.ref_log_value(bytes(data), len(data)))

    def read_from(img, off):
        b = np.ascontiguousarray(img, dtype=np.uint8)
        o = ctypes.create_string_buffer(1 << 22)
        k = ref.ref_log_read_from(b.ctypes.data, b.size, off, o, 1 << 22)
        return o.raw[:k].decode()

    payload = printable_bytes(SEED, 6 * BLOCK)
    scenarios = []
    for name, frame, edits, offsets in SCENARIOS:
        img = frame_image(frame, edits, payload, value)
        reads = [{"initial_offset": int(off), "events": read_from(img, int(off))} for off in [0] + list(offsets)]
        scenarios.append({"name": name, "frame": frame, "edits": edits, "bytes": int(img.size), "reads": reads})
    fixture = {
        "source": "lsbm common/log_reader.cc built from the reference (oracle/Makefile reflog); "
                  "tests/golden/make_logread_fixture.py",
        "seed": SEED, "payload_bytes": 6 * BLOCK, "scenarios": scenarios,
    }
    with open(os.path.join(HERE, "logread_fixture.json"), "w") as f:
        json.dump(fixture, f, indent=0)
    kinds = sorted({line.split(" ", 2)[2] if line.startswith("D") else "R"
                    for s in scenarios for r in s["reads"] for line in r["events"].splitlines()})
    print(f"{len(scenarios)} scenarios, {sum(len(s['reads']) for s in scenarios)} reads; event kinds: {kinds}")


if __name__ == "__main__":
    sys.exit(main())
