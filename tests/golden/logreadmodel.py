"""A plain Python model of the batched log::Reader (include/lsbm_log_read.h):
the three layers walk, plan and emit, each producing the arrays the C ABI
states, written as the serial loops of common/log_reader.cc (the device code
is scans; this is what they must equal).

    walk(buf, initial_offset)                -> Walk(block_first, block_end, headers)
    header_fields(buf, headers)              -> (stored masked CRC, offsets of [type || payload])
    plan(buf, w, ok, initial_offset)         -> Plan(records, events, side_bytes, stop)
    emit(buf, p, log_at, side_at)            -> Emit(records, last_record_offset, events, side)
    read(buf, ok_of, initial_offset, ...)    -> (Walk, Plan, Emit)
    event_text(e, record_crc)                -> the fixtures' R / D text

`ok` is one bool per header (ReadPhysicalRecord's checksum test); the model
does not compute CRCs itself.
"""
from collections import namedtuple

import numpy as np

BLOCK, HEADER = 32768, 7  # common/log_format.h
RAN_OUT, TRAILER, BAD_LENGTH, ZERO_HEADER, TRUNCATED = range(5)
REASONS = {1: "bad record length", 2: "checksum mismatch", 3: "truncated record at end of file",
           4: "partial record without end(1)", 5: "partial record without end(2)",
           6: "partial record without end(3)", 7: "missing start of fragmented record(1)",
           8: "missing start of fragmented record(2)", 9: "error in middle of record", 10: "unknown record type"}
M64 = (1 << 64) - 1

Walk = namedtuple("Walk", "block_first block_end headers")
Plan = namedtuple("Plan", "records events side_bytes stop")
Emit = namedtuple("Emit", "records last_record_offset events side")


def first_block(initial_offset):
    """SkipToInitialBlock (common/log_reader.cc:35-45)."""
    return initial_offset // BLOCK + (1 if initial_offset % BLOCK > BLOCK - 6 else 0)


def n_blocks(log_bytes, initial_offset):
    start = first_block(initial_offset) * BLOCK
    return 0 if start >= log_bytes else -(-(log_bytes - start) // BLOCK)


def walk(buf, initial_offset=0):
    """ReadPhysicalRecord's walk of every block from its own start, CRCs aside."""
    n, fb = len(buf), first_block(initial_offset)
    nb = n_blocks(n, initial_offset)
    block_first, block_end, headers = [0], [], []
    for r in range(nb):
        start = (fb + r) * BLOCK
        size = min(BLOCK, n - start)
        pos = 0
        while True:
            rem = size - pos
            if rem < HEADER:
                how = RAN_OUT if rem == 0 else (TRAILER if size == BLOCK else TRUNCATED)
                break
            length = int(buf[start + pos + 4]) | int(buf[start + pos + 5]) << 8
            if HEADER + length > rem:
                how = BAD_LENGTH
                break
            if buf[start + pos + 6] == 0 and length == 0:
                how = ZERO_HEADER
                break
            headers.append(start + pos)
            pos += HEADER + length
        block_first.append(len(headers))
        block_end.append((how, size - pos))
    return Walk(np.array(block_first, dtype=np.int64), np.array(block_end, dtype=np.int64).reshape(-1, 2),
                np.array(headers, dtype=np.int64))


def header_fields(buf, headers):
    """(the stored CRC field of every header, offsets[n + 1] and bytes of the
    concatenated [type || payload] ranges): what a CRC oracle needs for `ok`."""
    buf = np.asarray(buf, dtype=np.uint8)
    stored, parts = [], []
    for h in headers:
        h = int(h)
        length = int(buf[h + 4]) | int(buf[h + 5]) << 8
        stored.append(int.from_bytes(buf[h:h + 4].tobytes(), "little"))
        parts.append(buf[h + 6:h + 7 + length])
    offs = np.zeros(len(parts) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([p.size for p in parts])
    data = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return np.array(stored, dtype=np.uint32), offs, data


def plan(buf, w, ok, initial_offset=0):
    """ReadRecord's loop until it returns false.  records: ("full", payload
    offset, length, LastRecordOffset) or ("frag", [(offset, length)...], length,
    LastRecordOffset); events: (records returned before, bytes, reason, arg)."""
    n, init, fb = len(buf), initial_offset, first_block(initial_offset)
    records, events = [], []
    # "at": end_of_buffer_offset_ - buffer_.size() before ReadPhysicalRecord is called, which is
    # physical_record_offset: where the record before ended, a skipped trailer not yet behind it
    st = {"in": False, "scratch": 0, "frags": [], "first": 0, "at": fb * BLOCK}

    def drop(end, nbytes, reason, arg=0):  # ReportDrop's filter, unsigned 64-bit
        if (end - nbytes) & M64 >= init:
            events.append((len(records), nbytes, reason, arg))

    def bad(end):  # kBadRecord
        if st["in"]:
            drop(end, st["scratch"], 9)
        st["in"], st["scratch"], st["frags"] = False, 0, []

    def eof(end):  # kEof
        if st["in"]:
            drop(end, st["scratch"], 6)

    for r in range(len(w.block_end)):
        start = (fb + r) * BLOCK
        bend = start + min(BLOCK, n - start)
        cut = False
        for k in range(int(w.block_first[r]), int(w.block_first[r + 1])):
            o = int(w.headers[k])
            length, t = int(buf[o + 4]) | int(buf[o + 5]) << 8, int(buf[o + 6])
            if not ok[k]:  # the rest of the block goes, this header included
                drop(bend, bend - o, 2)
                bad(bend)
                st["at"] = bend
                cut = True
                break
            end = o + HEADER + length
            at, st["at"] = st["at"], end
            if o < init:  # a physical record that starts before initial_offset
                bad(end)
            elif t == 1:
                if st["in"] and st["scratch"]:
                    drop(end, st["scratch"], 4)
                st["in"], st["scratch"], st["frags"] = False, 0, []
                records.append(("full", o + HEADER, length, at))
            elif t == 2:
                if st["in"] and st["scratch"]:
                    drop(end, st["scratch"], 5)
                st["in"], st["scratch"], st["frags"], st["first"] = True, length, [(o + HEADER, length)], at
            elif t in (3, 4):
                if not st["in"]:
                    drop(end, length, 7 if t == 3 else 8)
                else:
                    st["scratch"] += length
                    st["frags"].append((o + HEADER, length))
                    if t == 4:
                        records.append(("frag", st["frags"], st["scratch"], st["first"]))
                        st["in"], st["scratch"], st["frags"] = False, 0, []
            elif t == 5:  # aliases kEof
                eof(end)
                return Plan(records, events, _side(records), o)
            elif t == 6:  # aliases kBadRecord
                bad(end)
            else:
                wide = t if t < 128 else t + 0xFFFFFF00  # a char widened to unsigned int
                drop(end, length + (st["scratch"] if st["in"] else 0), 10, wide)
                st["in"], st["scratch"], st["frags"] = False, 0, []
        if cut:
            continue
        how, rem = int(w.block_end[r][0]), int(w.block_end[r][1])
        if how == BAD_LENGTH:
            drop(bend, rem, 1)
            bad(bend)
            st["at"] = bend
        elif how == ZERO_HEADER:
            bad(bend)
            st["at"] = bend
        elif how == TRUNCATED:
            drop(bend, rem, 3)
    eof(n)
    return Plan(records, events, _side(records), n)


def _side(records):
    return sum(rec[2] for rec in records if rec[0] == "frag")


def emit(buf, p, log_at=0, side_at=None):
    """The plan written out: records int64[n, 2] with offsets in the image
    (log at log_at, side area at side_at, by default right after the log),
    last_record_offset int64[n], events int64[m, 4] (arg as the 64-bit value)
    and the side area's bytes."""
    buf = np.asarray(buf, dtype=np.uint8)
    if side_at is None:
        side_at = log_at + len(buf)
    recs, lro, side, at = [], [], [], 0
    for rec in p.records:
        if rec[0] == "full":
            recs.append((log_at + rec[1], rec[2]))
        else:
            recs.append((side_at + at, rec[2]))
            side += [buf[o:o + ln] for o, ln in rec[1]]
            at += rec[2]
        lro.append(rec[3])
    return Emit(np.array(recs, dtype=np.int64).reshape(-1, 2), np.array(lro, dtype=np.int64),
                np.array(p.events, dtype=np.int64).reshape(-1, 4),
                np.concatenate(side) if side else np.zeros(0, np.uint8))


def read(buf, ok_of, initial_offset=0, log_at=0, side_at=None):
    """walk, ok = ok_of(buf, headers), plan, emit."""
    buf = np.asarray(buf, dtype=np.uint8)
    w = walk(buf, initial_offset)
    p = plan(buf, w, ok_of(buf, w.headers), initial_offset)
    return w, p, emit(buf, p, log_at, side_at)


def record_bytes(buf, p):
    """Every record of a plan as bytes."""
    buf = np.asarray(buf, dtype=np.uint8)
    return [buf[rec[1]:rec[1] + rec[2]].tobytes() if rec[0] == "full" else
            b"".join(buf[o:o + ln].tobytes() for o, ln in rec[1]) for rec in p.records]


def event_text(e, payloads, value):
    """The text ref_log_read_from prints: R <length> <crc32c> <LastRecordOffset>
    and D <bytes> <status>, reports placed between the records."""
    lines, ev = [], e.events.tolist()
    for i in range(len(payloads) + 1):
        for before, nbytes, reason, arg in ev:
            if before == i:
                what = REASONS[reason] + (f" {arg & 0xFFFFFFFF}" if reason == 10 else "")
                lines.append(f"D {nbytes} Corruption: {what}")
        if i < len(payloads):
            lines.append(f"R {len(payloads[i])} {value(payloads[i]):08x} {int(e.last_record_offset[i])}")
    return "".join(line + "\n" for line in lines)


def mask(crc):
    """util/crc32c.h Mask."""
    return (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def apply_edits(img, edits):
    """The byte edits of tests/golden/log_fixture.json's scenarios."""
    img = np.array(img, dtype=np.uint8)
    for op in edits:
        if op[0] == "xor":
            img[op[1]] ^= op[2]
        elif op[0] == "set":
            b = np.frombuffer(bytes.fromhex(op[2]), np.uint8)
            img[op[1]:op[1] + b.size] = b
        elif op[0] == "zero":
            img[op[1]:op[1] + op[2]] = 0
        elif op[0] == "truncate":
            img = img[:op[1]]
    return img


def frame_image(frame, edits, payload, value):
    """A hand-framed log image (tests/golden/logread_fixture.json).  frame ops:
    ["p", type, length] one physical record with a valid CRC whose payload is
    the next `length` bytes of `payload`; ["p", type, length, present] the same
    with only `present` payload bytes in the file (its length field still says
    `length`); ["z", n] n zero bytes; ["x", n, op] op n times.  Then
    apply_edits.  value: crc32c."""
    out, at = [], 0
    for op in [o for f in frame for o in ([f[2]] * f[1] if f[0] == "x" else [f])]:
        if op[0] == "z":
            out.append(np.zeros(op[1], np.uint8))
            continue
        _, t, length = op[:3]
        present = op[3] if len(op) > 3 else length
        body = np.asarray(payload[at:at + present], dtype=np.uint8)
        at += present
        crc = mask(value(bytes([t]) + body.tobytes()))
        out.append(np.frombuffer(crc.to_bytes(4, "little") + bytes([length & 0xFF, length >> 8, t]), np.uint8))
        out.append(body)
    img = np.concatenate(out) if out else np.zeros(0, np.uint8)
    return apply_edits(img, edits)
