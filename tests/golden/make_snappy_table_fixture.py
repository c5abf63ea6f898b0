"""Writes tests/golden/snappy_tables.json + snappy_tables.bin: the table files
TableBuilder writes under options.compression = kSnappyCompression for the
cases of snappy_table_cases.py, computed by the plain-Python model
(snappytablemodel.py) with pyarrow's libsnappy as the codec.  Neither the oracle
nor the library takes part, so the fixture is independent of both; the tests
read the committed files and never import pyarrow.

    python tests/golden/make_snappy_table_fixture.py

Every case asserts the property it exists for and the run fails without it.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pyarrow  # noqa: E402

from golden import buildmodel as bd  # noqa: E402
from golden import snappy_table_cases as cases  # noqa: E402
from golden import snappytablemodel as stm  # noqa: E402

CODEC = pyarrow.Codec("snappy")


def compress(raw):
    return CODEC.compress(raw, asbytes=True)


def uncompress(comp):
    from golden.blockmodel import get_varint32
    pre = get_varint32(comp, 0, len(comp))
    if pre is None:
        return None
    try:
        return CODEC.decompress(comp, decompressed_size=pre[0], asbytes=True)
    except Exception:  # noqa: BLE001 (libsnappy's "corrupt input")
        return None


def changes(types):
    return sum(1 for a, b in zip(types, types[1:]) if a != b)


def check_case(name, params, entries, data, handles, types):
    cmp, block_size, restart_interval, bits_per_key = params
    plain, plain_handles, _ = bd.table_file(entries, cmp, block_size, restart_interval, bits_per_key)
    nd = len(handles)
    data_types, index_type = types[:nd], types[-1]
    back = stm.read_table(data, uncompress)
    assert back["entries"] == entries and back["types"] == types, name
    if name.startswith("mixed_"):
        # the types alternate, so every later offset differs from the uncompressed layout's
        assert changes(data_types) == nd - 1 and nd >= 4, (name, data_types)
        assert all(h[0] != p[0] for h, p in zip(handles[1:], plain_handles[1:])), name
    elif name == "all_compressible":
        assert data_types == [1] * nd and nd >= 4, (name, data_types)
    elif name == "none_compressible":
        assert types == [0] * len(types) and data == plain and nd >= 3, (name, types)
    elif name == "index_compressed":
        assert index_type == 1 and nd >= 300, (name, index_type, nd)
    elif name == "index_raw":
        assert index_type == 0 and nd >= 3, (name, index_type, nd)
    elif name == "bloom_internal":
        assert bits_per_key == 10 and handles[-1][0] // 2048 >= 3, (name, handles[-1])
        plain_filter = stm.read_table(plain, uncompress)["filter"]
        assert back["filter"] != plain_filter and 1 in data_types, name
    elif name == "one_entry":
        assert len(entries) == 1 and nd == 1, name
    elif name == "empty":
        assert not entries and nd == 0, name
    else:
        raise KeyError(name)


def main():
    blob = bytearray()
    out = {"codec": "libsnappy (pyarrow %s)" % pyarrow.__version__, "cases": [], "compaction": None}

    def put(data):
        at = len(blob)
        blob.extend(data)
        return {"offset": at, "length": len(data)}

    for name, params in cases.CASES.items():
        cmp, block_size, restart_interval, bits_per_key = params
        entries = cases.entries(name)
        data, handles, index_handle, types = stm.table_file(entries, cmp, block_size, restart_interval,
                                                            bits_per_key, compress)
        check_case(name, params, entries, data, handles, types)
        rec = put(data)
        rec.update(name=name, data_handles=[list(h) for h in handles], index_handle=list(index_handle), types=types)
        out["cases"].append(rec)

    c = cases.COMPACTION
    runs = cases.compaction_runs()
    inputs = []
    for run in runs:
        data, handles, index_handle, types = stm.table_file(run, c["cmp"], c["block_size"], c["restart_interval"],
                                                            c["bits_per_key"], compress)
        assert 1 in types[:len(handles)]
        rec = put(data)
        rec.update(data_handles=[list(h) for h in handles], index_handle=list(index_handle))
        inputs.append(rec)
    users = [set(k[:-8] for k, _ in run) for run in runs]
    assert users[0] & users[1] & users[2], "the runs must overlap"
    outputs = stm.compact(runs, c["cmp"], c["max_file_size"], c["drop"], c["smallest_snapshot"], c["bottom_level"],
                          c["block_size"], c["restart_interval"], c["bits_per_key"], compress)
    assert len(outputs) >= 3, len(outputs)
    merged = [e for o in outputs for e in stm.read_table(o, uncompress)["entries"]]
    assert 0 < len(merged) < sum(len(r) for r in runs), "the drop rule must drop something"
    assert not any(k[-8] == 0 for k, _ in merged), "the deletion is below the snapshot at the bottom level"
    # the cut over packed sizes is not the cut over raw sizes
    raw_cut = stm.compact(runs, c["cmp"], c["max_file_size"], c["drop"], c["smallest_snapshot"], c["bottom_level"],
                          c["block_size"], c["restart_interval"], c["bits_per_key"], None)
    assert len(raw_cut) != len(outputs), (len(raw_cut), len(outputs))
    out["compaction"] = {"inputs": inputs, "outputs": [put(o) for o in outputs]}

    assert len(blob) < 100_000, len(blob)
    with open(os.path.join(HERE, "snappy_tables.bin"), "wb") as f:
        f.write(bytes(blob))
    with open(os.path.join(HERE, "snappy_tables.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases, %d compaction outputs, %d bytes" % (len(out["cases"]), len(outputs), len(blob)))


if __name__ == "__main__":
    main()
