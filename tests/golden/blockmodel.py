"""Plain-Python restatement of lsbm's table/block.cc (Block, DecodeEntry,
Block::Iter forward iteration and Seek), table/block_builder.cc, both
comparators and BlockHandle::DecodeFrom -- the model the GPU block reader
(include/lsbm_block.h) is compared with.  tests/test_block.py pins it to the
reference's own results (tests/golden/block_fixture.json).

Statuses and states are those of include/lsbm_block.h.
"""
import hashlib
import struct

OK, BAD_CONTENTS, BAD_ENTRY, NO_ROOM = 0, 1, 2, 3
VALID, NOT_VALID, SEEK_BAD_ENTRY, SEEK_BAD_CONTENTS, SEEK_BAD_HANDLE = 0, 1, 2, 3, 4
BYTEWISE, INTERNAL_KEY = 0, 1
MESSAGE = {OK: "OK", BAD_CONTENTS: "Corruption: bad block contents",
           BAD_ENTRY: "Corruption: bad entry in block"}
SEEK_MESSAGE = {VALID: "OK", NOT_VALID: "OK", SEEK_BAD_ENTRY: "Corruption: bad entry in block",
                SEEK_BAD_CONTENTS: "Corruption: bad block contents",
                SEEK_BAD_HANDLE: "Corruption: bad block handle"}


class BadKey(Exception):
    """InternalKeyComparator on a key shorter than 8 bytes (the reference asserts)."""


def put_varint(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def get_varint32(b, p, limit):
    """GetVarint32Ptr (util/coding.cc:112-129): (value, next p) or None."""
    r, shift = 0, 0
    while shift <= 28 and p < limit:
        byte = b[p]
        p += 1
        if byte & 128:
            r |= (byte & 127) << shift
        else:
            return (r | (byte << shift)) & 0xFFFFFFFF, p
        shift += 7
    return None


def get_varint64(b, p, limit):
    r, shift = 0, 0
    while shift <= 63 and p < limit:
        byte = b[p]
        p += 1
        if byte & 128:
            r |= (byte & 127) << shift
        else:
            return (r | (byte << shift)) & 0xFFFFFFFFFFFFFFFF, p
        shift += 7
    return None


def decode_handle(v):
    """BlockHandle::DecodeFrom (table/format.cc:23-30): (offset, size) or None."""
    a = get_varint64(v, 0, len(v))
    if a is None:
        return None
    b = get_varint64(v, a[1], len(v))
    if b is None:
        return None
    return a[0], b[0]


def decode_entry(b, p, limit):
    """DecodeEntry (table/block.cc:111-132): (shared, non_shared, value_length,
    key offset) or None.  The last check adds without the reference's 32-bit
    wrap (include/lsbm_block.h)."""
    if p > limit or limit - p < 3:
        return None
    sh, ns, vl = b[p], b[p + 1], b[p + 2]
    if (sh | ns | vl) < 128:
        p += 3
    else:
        for i in range(3):
            r = get_varint32(b, p, limit)
            if r is None:
                return None
            if i == 0:
                sh = r[0]
            elif i == 1:
                ns = r[0]
            else:
                vl = r[0]
            p = r[1]
    if limit - p < ns + vl:
        return None
    return sh, ns, vl, p


def block_layout(b):
    """Block::Block (table/block.cc:23-41): (restarts_, num_restarts) or None
    for "bad block contents"."""
    size = len(b)
    if size < 4 or size >= 1 << 32:
        return None
    nr = struct.unpack_from("<I", b, size - 4)[0]
    if nr > (size - 4) // 4:
        return None
    return size - (1 + nr) * 4, nr


def restart_point(b, restarts, i):
    return struct.unpack_from("<I", b, restarts + 4 * i)[0]


def walk(b):
    """SeekToFirst, then Next until !Valid: (status, [(key, value offset, value
    length, entry offset)]); the entries before an error count."""
    lay = block_layout(b)
    if lay is None:
        return BAD_CONTENTS, []
    restarts, nr = lay
    out = []
    if nr == 0:
        return OK, out
    p, key = restart_point(b, restarts, 0), b""
    while p < restarts:
        e = decode_entry(b, p, restarts)
        if e is None or len(key) < e[0]:
            return BAD_ENTRY, out
        sh, ns, vl, kp = e
        key = key[:sh] + bytes(b[kp:kp + ns])
        out.append((key, kp + ns, vl, p))
        p = kp + ns + vl
    return OK, out


def compare(a, b, cmp):
    """<0, 0, >0 (util/comparator.cc bytewise; common/dbformat.cc:50-66)."""
    if cmp == BYTEWISE:
        return (a > b) - (a < b)
    if len(a) < 8 or len(b) < 8:
        raise BadKey()
    ua, ub = a[:-8], b[:-8]
    if ua != ub:
        return (ua > ub) - (ua < ub)
    ta, tb = struct.unpack("<Q", a[-8:])[0], struct.unpack("<Q", b[-8:])[0]
    return -1 if ta > tb else (1 if ta < tb else 0)


def seek(b, target, cmp=BYTEWISE, value_is_handle=False):
    """Block::Iter::Seek (table/block.cc:223-265).  Returns a dict: state, pos
    (current_), key, value_offset, value_length, and handle with
    value_is_handle."""
    r = {"state": NOT_VALID, "pos": 0, "key": b"", "value_offset": 0, "value_length": 0,
         "handle": (0, 0)}
    lay = block_layout(b)
    if lay is None:
        r["state"] = SEEK_BAD_CONTENTS
        return r
    restarts, nr = lay
    if nr == 0:
        r["pos"] = len(b) - 4
        return r
    r["pos"] = restarts
    try:
        left, right = 0, nr - 1
        while left < right:
            mid = (left + right + 1) // 2
            e = decode_entry(b, restart_point(b, restarts, mid), restarts)
            if e is None or e[0] != 0:
                r["state"] = SEEK_BAD_ENTRY
                return r
            if compare(bytes(b[e[3]:e[3] + e[1]]), target, cmp) < 0:
                left = mid
            else:
                right = mid - 1
        p, key = restart_point(b, restarts, left), b""
        while p < restarts:
            e = decode_entry(b, p, restarts)
            if e is None or len(key) < e[0]:
                r["state"] = SEEK_BAD_ENTRY
                return r
            sh, ns, vl, kp = e
            key = key[:sh] + bytes(b[kp:kp + ns])
            if compare(key, target, cmp) >= 0:
                r.update(state=VALID, pos=p, key=key, value_offset=kp + ns, value_length=vl)
                if value_is_handle:
                    h = decode_handle(bytes(b[kp + ns:kp + ns + vl]))
                    if h is None:
                        r["state"] = SEEK_BAD_HANDLE
                    else:
                        r["handle"] = h
                return r
            p = kp + ns + vl
    except BadKey:
        r["state"] = SEEK_BAD_ENTRY
    return r


def entries_sha(b, entries):
    """SHA-256 over [u32 key length][key][u32 value length][value] of every entry."""
    h = hashlib.sha256()
    for key, vo, vl, _ in entries:
        h.update(struct.pack("<I", len(key)) + key + struct.pack("<I", vl) + bytes(b[vo:vo + vl]))
    return h.hexdigest()


def build_block(entries, restart_interval=16):
    """BlockBuilder (table/block_builder.cc): Add for every (key, value), Finish."""
    buf, restarts, counter, last = bytearray(), [0], 0, b""
    for key, value in entries:
        shared = 0
        if counter < restart_interval:
            m = min(len(last), len(key))
            while shared < m and last[shared] == key[shared]:
                shared += 1
        else:
            restarts.append(len(buf))
            counter = 0
        buf += put_varint(shared) + put_varint(len(key) - shared) + put_varint(len(value))
        buf += key[shared:] + value
        last = key
        counter += 1
    for r in restarts:
        buf += struct.pack("<I", r)
    buf += struct.pack("<I", len(restarts))
    return bytes(buf)


def seek_targets(keys):
    """The probes of the fixture: every key, every key with its last byte -1
    and +1, every key truncated by one and to half, the empty target and one
    target above all keys."""
    t = []
    for k in keys:
        t.append(k)
        if k:
            t.append(k[:-1] + bytes([(k[-1] - 1) & 255]))
            t.append(k[:-1] + bytes([(k[-1] + 1) & 255]))
            t.append(k[:-1])
            t.append(k[:len(k) // 2])
    t.append(b"")
    t.append(b"\xff" * 40)
    return t
