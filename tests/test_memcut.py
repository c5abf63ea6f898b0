"""The memtable switch's model (tests/golden/memcutmodel.py) against the
reference's recorded accounting (tests/golden/memcut_fixture.*), against a
literal per-allocation restatement, and through its state; and the host
baseline's self-check (tools/memcut_host.cc).  CPU only.
"""
import json
import os
import random
import shutil
import subprocess
import zlib

import pytest

from golden import memcut_cases as cases
from golden import memcutmodel as mm

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def load_fixture():
    index = json.load(open(os.path.join(HERE, "golden", "memcut_fixture.json")))
    text = zlib.decompress(open(os.path.join(HERE, "golden", "memcut_fixture.bin"), "rb").read())
    assert len(text) == index["bin"]["inflated"] and zlib.crc32(text) == index["bin"]["crc32"]
    return index, json.loads(text)


INDEX, FIXTURE = load_fixture()
SCENARIOS = sorted(FIXTURE["scenarios"])


def want_of(cutrec, n_records):
    """The fixture's record of one run in cut()'s shape."""
    n_mem = len(cutrec["mem_first"])
    return dict(usage=cutrec["usage"], mem_first=cutrec["mem_first"] + [n_records], mem_usage=cutrec["ended"],
                n_mem=n_mem, have_mem=cutrec["open_at_end"])


def check_against(got, cutrec, n_records):
    want = want_of(cutrec, n_records)
    assert got["status"] == mm.OK
    assert got["usage"] == want["usage"]
    assert got["mem_first"] == want["mem_first"]
    assert got["mem_usage"] == want["mem_usage"]
    assert got["counts"] == [want["n_mem"], 0]
    assert got["state"][0] == want["have_mem"]


def test_fixture_covers_the_cases():
    assert sorted(n for n, _ in cases.scenarios()) == SCENARIOS
    assert INDEX["write_buffer_sizes"] == list(cases.WRITE_BUFFER_SIZES)
    assert FIXTURE["scenarios"]["empty_batch"]["cuts"]["recover_65536"]["usage"] == [mm.FRESH_USAGE]
    assert max(INDEX["scenarios"][s]["memtables"]["recover_65536"] for s in SCENARIOS) >= 5
    assert FIXTURE["scenarios"]["cut_on_last"]["cuts"]["recover_65536"]["open_at_end"] == 0
    assert FIXTURE["scenarios"]["cut_on_last"]["cuts"]["write_65536"]["open_at_end"] == 1
    # 16 standard blocks: the vector's capacity decides at 65,600, not yet at 65,664
    b = FIXTURE["scenarios"]["blocks_33"]["cuts"]
    assert 65536 + 128 in b["recover_65600"]["ended"] and 65536 + 128 not in b["recover_65664"]["ended"]
    st = FIXTURE["scenarios"]["records_in_error"]["status"]
    assert {1, 2, 4, 5} <= set(st)


def test_heights_match_the_reference():
    for name, run in FIXTURE["heights"].items():
        got, rnd = mm.heights(run["rnd"], len(run["heights"]))
        assert got == run["heights"], name
        assert rnd == run["rnd_after"], name
    assert FIXTURE["heights"]["first_2000"]["rnd"] == mm.SEED
    h12 = FIXTURE["heights"]["height_12"]["heights"]
    assert 12 in h12 and h12.index(12) + 1 < len(h12)
    # the reference's own Random: the first height 12 from the fixed seed
    assert FIXTURE["first_height_12"] == {"insert": cases.HEIGHT12_INSERT, "draws": cases.HEIGHT12_DRAW}
    assert (cases.HEIGHT12_INSERT, cases.HEIGHT12_DRAW) == (1003046, 1338279)


@pytest.mark.parametrize("name", SCENARIOS)
def test_model_reproduces_the_fixture(name):
    s = FIXTURE["scenarios"][name]
    entries, base = cases.entries_of(s["ops"])
    for w in cases.WRITE_BUFFER_SIZES:
        for mode, key in ((mm.RECOVER, "recover"), (mm.WRITE, "write")):
            got = mm.cut(entries, base, s["status"], mode, w)
            check_against(got, s["cuts"][f"{key}_{w}"], len(s["ops"]))


def test_cases_are_what_the_reference_decoded():
    """The scenarios' reps, decoded by the reference, are the ops the cases meant."""
    recorded = {n: FIXTURE["scenarios"][n] for n in SCENARIOS}
    assert recorded["one_record_257"]["ops"] == [[[16, 100, 1]] * 257]
    assert [len(o) for o in recorded["records_in_error"]["ops"]][60] == 2  # the bad Put keeps two entries


class LiteralArena:
    """util/arena.cc with addresses: blocks at multiples of 16, as new char[] gives them."""

    def __init__(self):
        self.ptr, self.left, self.blocks, self.bytes, self.next_block = 0, 0, 0, 0, 1 << 20

    def _block(self, n):
        at = self.next_block
        self.next_block += (n + 15) // 16 * 16 + 16
        self.blocks += 1
        self.bytes += n
        return at

    def _fallback(self, n):
        if n > 1024:
            return self._block(n)
        self.ptr, self.left = self._block(4096), 4096
        return self._take(n)

    def _take(self, n):
        self.ptr, self.left = self.ptr + n, self.left - n
        return self.ptr - n

    def plain(self, n):
        return self._take(n) if n <= self.left else self._fallback(n)

    def aligned(self, n):
        slop = -self.ptr % 8
        if n + slop <= self.left:
            return self._take(n + slop) + slop
        return self._fallback(n)

    def usage(self):
        cap = 1
        while cap < self.blocks:  # push_back's doubling
            cap *= 2
        return self.bytes + 8 * (cap if self.blocks else 0)


def literal(entries, base, status, mode, wbs):
    usage, first, ended, mem, last, rnd = [], [], [], None, 0, 0
    for i in range(len(base) - 1):
        if mode == mm.RECOVER and status[i] in mm.WB_SKIPPED:
            usage.append(last)
            continue
        if mode == mm.WRITE and mem is not None and mem.usage() > wbs:
            ended.append(mem.usage())
            mem = None
        if mem is None:
            mem, rnd = LiteralArena(), mm.SEED
            assert mem.aligned(104) % 8 == 0
            first.append(i)
        for ikl, vl, t in entries[base[i]:base[i + 1]]:
            mem.plain(mm.entry_size(ikl, vl if t else 0))
            h = 1
            while h < 12:
                rnd = rnd * 16807 % 2147483647
                if rnd % 4:
                    break
                h += 1
            assert mem.aligned(8 + 8 * h) % 8 == 0
        last = mem.usage()
        usage.append(last)
        if mode == mm.RECOVER and last > wbs:
            ended.append(last)
            mem, last = None, 0
    if mem is not None:
        ended.append(mem.usage())
    return usage, first, ended


def random_history(rng, n_records):
    entries, base, status = [], [0], []
    for _ in range(n_records):
        roll = rng.randrange(16)
        status.append(1 if roll == 0 else 2 if roll == 1 else 0)
        for _ in range(0 if status[-1] == 1 else rng.choice((0, 1, 1, 2, 5, 40))):
            t = int(rng.randrange(8) > 0)
            entries.append((8 + rng.randrange(41), rng.choice((0, 10, 100, 100, 900, 1000, 1100, 3000, 17000))
                            + rng.randrange(9), t))
        base.append(len(entries))
    return entries, base, status


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_the_literal_restatement(seed):
    rng = random.Random(seed)
    entries, base, status = random_history(rng, 150)
    for w in cases.WRITE_BUFFER_SIZES:
        for mode in (mm.RECOVER, mm.WRITE):
            got = mm.cut(entries, base, status, mode, w)
            usage, first, ended = literal(entries, base, status, mode, w)
            assert (got["usage"], got["mem_first"][:-1], got["mem_usage"]) == (usage, first, ended)


def joined(a, b, at):
    """Two calls' results as one call's."""
    first, ended = a["mem_first"][:-1], list(a["mem_usage"])
    for k in range(b["counts"][0]):
        if k == 0 and b["counts"][1]:
            ended[-1] = b["mem_usage"][0]
        else:
            first.append(b["mem_first"][k] + at)
            ended.append(b["mem_usage"][k])
    return a["usage"] + b["usage"], first, ended, b["state"]


@pytest.mark.parametrize("seed", range(3))
def test_two_calls_through_the_state_equal_one(seed):
    rng = random.Random(100 + seed)
    entries, base, status = random_history(rng, 40)
    n = len(base) - 1
    for w in (4104, 8192, 65536):
        for mode in (mm.RECOVER, mm.WRITE):
            one = mm.cut(entries, base, status, mode, w)
            for at in range(n + 1):
                a = mm.cut(entries[:base[at]], base[:at + 1], status[:at], mode, w)
                b = mm.cut(entries[base[at]:], [x - base[at] for x in base[at:]], status[at:], mode, w, a["state"])
                assert joined(a, b, at) == (one["usage"], one["mem_first"][:-1], one["mem_usage"], one["state"])


def test_model_refuses_bad_input():
    e, b = [(16, 10, 1)] * 3, [0, 1, 3]
    assert mm.cut(e, b, None, mm.RECOVER, 4103)["status"] == mm.BAD_INPUT
    assert mm.cut(e, [0, 2, 1, 3], None, mm.RECOVER, 65536)["status"] == mm.BAD_INPUT
    assert mm.cut(e, [1, 3], None, mm.RECOVER, 65536)["status"] == mm.BAD_INPUT
    assert mm.cut(e, [0, 2], None, mm.RECOVER, 65536)["status"] == mm.BAD_INPUT
    assert mm.cut([(16, 10, 2)], [0, 1], None, mm.WRITE, 65536)["status"] == mm.BAD_INPUT
    assert mm.cut([(1 << 32, 10, 1)], [0, 1], None, mm.WRITE, 65536)["status"] == mm.BAD_INPUT
    for st in ([1, 4104, 1, 4096, mm.SEED, 0], [1, 12, 1, 4096, mm.SEED, 0], [1, 8, 0, 0, mm.SEED, 0],
               [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, mm.M, 0], [2, 0, 1, 4096, mm.SEED, 0]):
        assert mm.cut(e, b, None, mm.WRITE, 65536, st)["status"] == mm.BAD_INPUT
    assert mm.cut(e, b, None, mm.RECOVER, 4104, mem_cap=0)["status"] == mm.NO_ROOM


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_baseline_self_check(tmp_path):
    exe = tmp_path / "memcut_host_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-DMEMCUT_HOST_MAIN", "-o", str(exe),
                    os.path.join(REPO, "tools", "memcut_host.cc")], check=True, timeout=300)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=300).stdout
    assert "memcut_host self-check ok" in out
