"""The batched log::Reader's Python model (tests/golden/logreadmodel.py: walk,
plan, emit with the arrays of include/lsbm_log_read.h) against the reference's
own log::Reader: all 46 scenarios of tests/golden/log_fixture.json (25
corruptions, 21 initial offsets) and every read of the hand-framed images of
tests/golden/logread_fixture.json.  Compared: the full event text -- every
record's length, CRC (by the oracle) and LastRecordOffset, every
Reporter::Corruption call, in order.  CPU only; the device is held to the same
model in tests/test_log_read_gpu.py.
"""
import json
import os

import numpy as np
import pytest

from golden import logreadmodel as model
from golden.splitmix import printable_bytes

HERE = os.path.dirname(os.path.abspath(__file__))


def load(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def wal_image(d):
    """The reference writer's image of log_fixture.json: the framing of its
    records with the fixture's header CRCs."""
    from lsbm_amd import log
    lens = d["lens"]
    payload = printable_bytes(d["seed"], int(sum(lens)))
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    img, heads = log.layout_records(payload[offs[i]:offs[i + 1]] for i in range(len(lens)))
    for h, c in zip(heads.tolist(), d["image"]["header_crcs"]):
        img[h:h + 4] = np.frombuffer(bytes.fromhex(c), np.uint8)
    assert img.size == d["image"]["bytes"]
    return img


def ok_by(oracle):
    def ok_of(buf, headers):
        stored, offs, data = model.header_fields(buf, headers)
        return oracle.batch_offsets(data, offs, masked=True) == stored
    return ok_of


def model_text(oracle, img, initial_offset):
    w, p, e = model.read(img, ok_by(oracle), initial_offset)
    assert len(e.records) == len(p.records) and e.side.size == p.side_bytes
    return model.event_text(e, model.record_bytes(img, p), oracle.value)


@pytest.fixture(scope="module")
def wal():
    d = load("log_fixture.json")
    return d, wal_image(d)


def test_model_matches_reference_on_the_wal_fixture(wal, oracle):
    d, base = wal
    assert oracle.value(base.tobytes()) == d["image"]["crc32c"]
    assert len(d["scenarios"]) == 25 and len(d["offset_scenarios"]) == 21
    failed = []
    for s in d["scenarios"] + d["offset_scenarios"]:
        got = model_text(oracle, model.apply_edits(base, s["ops"]), s.get("initial_offset", 0))
        if got != s["events"]:
            failed.append(s["name"])
    assert not failed, failed


def test_model_matches_reference_on_the_hand_framed_images(oracle):
    d = load("logread_fixture.json")
    payload = printable_bytes(d["seed"], d["payload_bytes"])
    failed = []
    for s in d["scenarios"]:
        img = model.frame_image(s["frame"], s["edits"], payload, oracle.value)
        assert img.size == s["bytes"]
        for r in s["reads"]:
            if model_text(oracle, img, r["initial_offset"]) != r["events"]:
                failed.append((s["name"], r["initial_offset"]))
    assert not failed, failed


def test_the_cases_the_issue_states(oracle):
    """The six reads checked by hand against the reference."""
    d = {s["name"]: s for s in load("logread_fixture.json")["scenarios"]}
    first = {k: s["reads"][0]["events"].splitlines() for k, s in d.items()}
    assert first["empty"] == []
    assert first["three_bytes"] == ["D 3 Corruption: truncated record at end of file"]
    assert [x.split()[0::3] for x in first["quirk_full"]] == [["R", "0"], ["R", "32768"]]
    assert [x.split()[0::3] for x in first["quirk_middle_last"]] == [["R", "0"], ["R", "32761"]]
    assert first["five_blocks_third_zeroed"] == [
        "D 65522 Corruption: error in middle of record",
        "D 32761 Corruption: missing start of fragmented record(1)",
        "D 10 Corruption: missing start of fragmented record(2)"]
    assert len(first["block_of_empty_records"]) == 4682 and all(x[0] == "R" for x in first["block_of_empty_records"])


def test_model_arrays_have_the_abi_shapes(wal, oracle):
    """walk's arrays are what plan verifies: block_first partitions the headers,
    every header chain starts at its block's start, the ends add up."""
    d, base = wal
    for off in (0, 40000, model.BLOCK - 5):
        w, p, e = model.read(base, ok_by(oracle), off)
        nb = model.n_blocks(base.size, off)
        assert w.block_first.size == nb + 1 and w.block_end.shape == (nb, 2)
        assert w.block_first[0] == 0 and w.block_first[-1] == w.headers.size
        fb = model.first_block(off)
        for r in range(nb):
            hs = w.headers[w.block_first[r]:w.block_first[r + 1]]
            assert hs.size == 0 or hs[0] == (fb + r) * model.BLOCK
        assert e.records.shape == (len(p.records), 2) and e.events.shape == (len(p.events), 4)
        assert e.last_record_offset.size == len(p.records)
        assert p.stop == base.size
