"""The batched VersionEdit at offsets past 4 GiB (arranged like
tests/test_high_offsets.py, whose constants it shares): one record decoded at
an offset past 2^32 in a sparse arena, with a decoy record of the same length
2^32 below it, and edits encoded to an out_at past 2^32 with guard bytes
there and at out_at - 2^32.  A kernel that drops the high half of an offset
decodes the decoy or writes the low place.
"""
import pytest

from golden import manifest_cases as cases
from golden import manifestmodel as mm
from high_offsets import ARENA_BYTES, FILL, GUARD, LINE
from test_manifest_gpu import dev, device_edits, host_edits, i64, tobytes

pytestmark = pytest.mark.gpu


class Sparse:
    """The arena's bytes where the test put some: {base: bytes}, sliced by absolute offsets."""

    def __init__(self, parts):
        self.parts = parts

    def __getitem__(self, s):
        for base, b in self.parts.items():
            if base <= s.start and s.stop <= base + len(b):
                return b[s.start - base:s.stop - base]
        raise IndexError(s)


def test_decode_and_encode_past_4gib(torch_cuda):
    from lsbm_amd import manifest as mf
    torch = torch_cuda
    rec = cases.all_tags() + cases.chain(300, 6)
    # a well-formed record of the same length: two-byte groups, one of three bytes where the length is odd
    other = (mm.put_varint(2) + mm.put_varint(300)) * (len(rec) % 2)
    other += (mm.put_varint(4) + mm.put_varint(1)) * ((len(rec) - len(other)) // 2)
    assert len(other) == len(rec) and mm.decode(other)[0] == 0 and mm.decode(other) != mm.decode(rec)
    arena = torch.empty(ARENA_BYTES, dtype=torch.uint8, device="cuda")
    at = LINE + 4099
    arena[at:at + len(rec)] = dev(torch, rec)
    arena[at - LINE:at - LINE + len(rec)] = dev(torch, other)
    E = mf.decode_edits(arena, i64(torch, [[at - LINE, len(rec)], [at, len(rec)]], 2))
    assert E.fields[1, mf.CMP_OFF].item() > LINE  # the comparator's offset is the image's
    assert host_edits(E, Sparse({at - LINE: other, at: rec})) == [mm.decode(other), mm.decode(rec)]
    # ---- encode to an out_at past the line
    edits = [e for _, e in cases.edits()[:6]]
    d = device_edits(torch, edits)
    d["del_first"], d["del_items"] = mf.sort_deleted(d["del_items"], len(edits))
    want_bytes = b"".join(mm.encode(e) for e in edits)
    out_at = LINE + (1 << 25) + 5
    for base in (out_at, out_at - LINE):
        arena[base - GUARD:base + len(want_bytes) + GUARD].fill_(FILL)
    args = (d["fields"], d["names"], d["del_first"], d["del_items"], d["new_first"], d["new_items"], d["keys"],
            d["key_offsets"])
    p = mf.encode_plan(*args, out_at)
    assert p.status.item() == 0 and p.totals.item() == len(want_bytes)
    assert p.records.cpu().tolist()[0] == [out_at, len(mm.encode(edits[0]))]
    assert mf.encode_emit(*args, p, arena, out_at, len(want_bytes)).item() == 0
    assert tobytes(arena[out_at - GUARD:out_at + len(want_bytes) + GUARD]) == (
        bytes([FILL]) * GUARD + want_bytes + bytes([FILL]) * GUARD)
    low = out_at - LINE
    assert (arena[low - GUARD:low + len(want_bytes) + GUARD] == FILL).all()
