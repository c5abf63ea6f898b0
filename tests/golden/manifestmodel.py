"""Plain-Python model of the MANIFEST engine (include/lsbm_manifest.h):
VersionEdit::DecodeFrom line by line (lsbm/version_edit.cc:137-251),
VersionEdit::EncodeTo (:51-114), and BasicVersionSet::Recover's loop with
Builder::Apply and MaybeAddFile's test (lsbm/version_set.cc:1987-2116,
:1660-1683, :1795) on an empty base.

An edit is a dict:
  comparator bytes or None; log_number, prev_log_number, next_file,
  last_sequence: int or None; write_cursor: int or None; read_cursors: four
  int-or-None; deleted: [(type, level, number)] and new: [(type, level,
  number, file_size, smallest, largest)], both in order of appearance.
"""
MESSAGES = {1: "comparator name", 2: "log number", 3: "previous log number", 4: "next file number",
            5: "last sequence number", 6: "deleted file", 7: "new-file entry", 8: "write cursor", 9: "read cursor",
            10: "unknown tag", 11: "invalid tag", 12: "file type out of range", 13: "read cursor index out of range"}
K_LEVELS = 4
BYTEWISE = b"leveldb.BytewiseComparator"
M64 = (1 << 64) - 1


def status_string(code):
    return "OK" if code == 0 else "Corruption: VersionEdit: " + MESSAGES[code]


def put_varint(v):
    out = bytearray()
    while v >= 128:
        out.append(v & 127 | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def put_slice(b):
    return put_varint(len(b)) + bytes(b)


def get_varint(buf, p, bits):
    """GetVarint32Ptr / GetVarint64Ptr: (value, next p) or None.  At most 5 /
    10 bytes; the last byte's bits that do not fit are lost."""
    r, shift = 0, 0
    while shift <= (28 if bits == 32 else 63) and p < len(buf):
        byte = buf[p]
        p += 1
        if byte & 128:
            r |= (byte & 127) << shift
        else:
            return (r | byte << shift) & ((1 << bits) - 1), p
        shift += 7
    return None


def get_slice(buf, p):
    g = get_varint(buf, p, 32)
    if g is None or len(buf) - g[1] < g[0]:
        return None
    return buf[g[1]:g[1] + g[0]], g[1] + g[0]


def empty_edit():
    return {"comparator": None, "log_number": None, "prev_log_number": None, "next_file": None, "last_sequence": None,
            "write_cursor": None, "read_cursors": [None] * 4, "deleted": [], "new": []}


def decode(buf):
    """(verdict, edit): DecodeFrom over one record.  A verdict other than 0
    comes with an empty edit."""
    buf = bytes(buf)
    e, p, code = empty_edit(), 0, 0
    numbers = {2: ("log_number", 2), 9: ("prev_log_number", 3), 3: ("next_file", 4), 4: ("last_sequence", 5),
               10: ("write_cursor", 8)}
    while code == 0:
        g = get_varint(buf, p, 32)
        if g is None:
            break
        tag, p = g
        if tag == 1:
            s = get_slice(buf, p)
            if s is None:
                code = 1
            else:
                e["comparator"], p = s
        elif tag in numbers:
            g = get_varint(buf, p, 64)
            if g is None:
                code = numbers[tag][1]
            else:
                e[numbers[tag][0]], p = g
        elif tag in (6, 7):
            vals, ok = [], True
            for what in ("type", "level", "number", "size", "key", "key")[:4 if tag == 6 else 6]:
                if what == "number" and tag == 6:
                    g = get_varint(buf, p, 64)
                elif what == "key":
                    g = get_slice(buf, p)
                else:
                    g = get_varint(buf, p, 32 if what in ("type", "level") else 64)
                if g is None or (what == "level" and g[0] >= K_LEVELS):
                    ok = False
                    break
                vals.append(g[0])
                p = g[1]
                if tag == 6 and what == "number":
                    break
            if not ok:
                code = tag
            elif vals[0] >= 4:
                code = 12  # the reference indexes a 4-element array with it
            else:
                e["deleted" if tag == 6 else "new"].append(tuple(vals))
        elif tag == 11:
            g = get_varint(buf, p, 64)
            if g is None:
                code = 9
            elif g[0] >= K_LEVELS:
                code = 13  # the reference indexes read_cursor_[4] with it
            else:
                i, p = g
                g = get_varint(buf, p, 64)
                if g is None:
                    code = 9
                else:
                    e["read_cursors"][i], p = g
        else:
            code = 10
    if code == 0 and p != len(buf):
        code = 11
    return (code, e) if code == 0 else (code, empty_edit())


def canonical(e):
    """The edit as the reference holds it after DecodeFrom and writes it back:
    deleted files a set per type, cursors that are absent 0."""
    c = dict(e)
    c["deleted"] = sorted(set(e["deleted"]))
    c["new"] = sorted(e["new"], key=lambda f: f[0])  # (stable: appearance order inside a type)
    c["write_cursor"] = e["write_cursor"] or 0
    c["read_cursors"] = [v or 0 for v in e["read_cursors"]]
    return c


def encode(e):
    """EncodeTo of canonical(e)."""
    e = canonical(e)
    out = bytearray()
    if e["comparator"] is not None:
        out += put_varint(1) + put_slice(e["comparator"])
    for tag, name in ((2, "log_number"), (9, "prev_log_number"), (3, "next_file"), (4, "last_sequence")):
        if e[name] is not None:
            out += put_varint(tag) + put_varint(e[name])
    for t in range(4):
        for (tt, level, number) in e["deleted"]:
            if tt == t:
                out += put_varint(6) + put_varint(t) + put_varint(level) + put_varint(number)
        for (tt, level, number, size, smallest, largest) in e["new"]:
            if tt == t:
                out += (put_varint(7) + put_varint(t) + put_varint(level) + put_varint(number) + put_varint(size)
                        + put_slice(smallest) + put_slice(largest))
    out += put_varint(10) + put_varint(e["write_cursor"])
    for i in range(4):
        out += put_varint(11) + put_varint(i) + put_varint(e["read_cursors"][i])
    return bytes(out)


def snapshot_edit(files, comparator=BYTEWISE, log_number=0, prev_log_number=0, next_file=0, last_sequence=0,
                  write_cursor=0, read_cursors=(0, 0, 0, 0)):
    """WriteSnapshot's edit: files are (type, level, number, size, smallest,
    largest), added level by level and inside a level type by type."""
    e = empty_edit()
    e.update(comparator=comparator, log_number=log_number, prev_log_number=prev_log_number, next_file=next_file,
             last_sequence=last_sequence, write_cursor=write_cursor, read_cursors=list(read_cursors))
    e["new"] = sorted(files, key=lambda f: (f[1], f[0]))
    return e


def live_files(edits):
    """Builder::Apply per edit, then MaybeAddFile's test, literally: per
    (level, type) a deleted set and an added list."""
    deleted, added = {}, {}
    for e in edits:
        e = canonical(e)
        for t in range(4):
            for (tt, level, number) in e["deleted"]:
                if tt == t:
                    deleted.setdefault((level, t), set()).add(number)
            for f in e["new"]:
                if f[0] == t:
                    deleted.setdefault((f[1], t), set()).discard(f[2])
                    added.setdefault((f[1], t), []).append(f[2:])
    out = {}
    for part, fs in added.items():
        keep = [f for f in fs if f[0] not in deleted.get(part, ())]
        if keep:
            out[part] = keep
    return out


def live_rule(edits):
    """The same by the closed rule the device folds with: an added entry is
    live iff the last record that adds its (type, level, number) is not before
    the last record that deletes it."""
    last_add, last_del = {}, {}
    for r, e in enumerate(edits):
        for (t, level, number) in e["deleted"]:
            last_del[(t, level, number)] = r
        for f in e["new"]:
            last_add[f[:3]] = r
    out = {}
    for e in edits:
        for f in sorted(e["new"], key=lambda f: f[0]):
            if last_add[f[:3]] >= last_del.get(f[:3], -1):
                out.setdefault((f[1], f[0]), []).append(f[2:])
    return out


def recover(records, events=(), comparator=BYTEWISE):
    """BasicVersionSet::Recover's loop over the records a log::Reader returns
    and its Reporter::Corruption events ((records before, status text)).
    Returns a dict: status and, where it is OK, the numbers and the live files."""
    k = min(len(records), events[0][0]) if events else len(records)
    edits = []
    for rec in records[:k]:
        code, e = decode(rec)
        if code:
            return {"status": status_string(code)}
        if e["comparator"] is not None and e["comparator"] != comparator:
            return {"status": "Invalid argument: " + e["comparator"].decode("latin-1")
                    + " does not match existing comparator : " + comparator.decode("latin-1")}
        edits.append(e)
    if events:
        return {"status": events[0][1]}

    def last(name):
        for e in reversed(edits):
            if e[name] is not None:
                return e[name]
        return None
    if last("next_file") is None:
        return {"status": "Corruption: no meta-nextfile entry in descriptor"}
    if last("log_number") is None:
        return {"status": "Corruption: no meta-lognumber entry in descriptor"}
    if last("last_sequence") is None:
        return {"status": "Corruption: no last-sequence-number entry in descriptor"}
    return {"status": "OK", "log_number": last("log_number"), "prev_log_number": last("prev_log_number") or 0,
            "manifest_file_number": last("next_file"), "next_file_number": (last("next_file") + 1) & M64,
            "last_sequence": last("last_sequence"), "files": live_files(edits)}
