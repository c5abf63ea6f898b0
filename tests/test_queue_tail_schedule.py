"""The cross-XCC work queue's late start (crc32c_units.h WgQueue own_rows, used
by crc32c_fixed_kernel), restated step for step on the CPU and run under random
interleavings of the waves, the way tests/test_queue_schedule.py restates the
full queue.

With own_rows = K0 >= 1 a workgroup's W waves take slots k = W, W+1, ... from an
LDS counter (slots 0 .. W-1 are the waves' own groups of row 0):
  * k < K0 W is a static slot: group (k / W) nwaves + W wg + k % W, with no
    global traffic, no ring entry and no publication (a group past the batch's
    end is skipped and the wave takes its next slot);
  * k >= K0 W is wave-group k % W of batch k / W - K0 + 1, whose item `it`
    covers the groups K0 nwaves + it W + [0, W).
Batch 1 is published by the wave that takes slot 0 of row K0 - 1 (K0 = 1: wave
0 at its own first group, the full queue), batch b + 1 by the wave that takes
slot 0 of batch b.  The heads, the batch-order rule, the ring rule and the end
(the first exhausted batch) are the full queue's.  Checked: every group is
processed exactly once, no ring entry is overwritten before all W readers read
it, and every wave stops.  K0 = 1 takes the same steps as
tests/test_queue_schedule.py's simulate().
"""
import os
import random
import re

import pytest

NONE = -1
LEAD = 1


def simulate(ngroups, nwg, W, own_rows, ring, seed):
    assert own_rows >= 1
    rnd = random.Random(seed)
    nwaves = nwg * W
    own_groups = own_rows * nwaves
    items = (ngroups - own_groups + W - 1) // W if ngroups > own_groups else 0
    heads = [0] * 8
    seen = [0] * ngroups
    claims = [0]  # global head claims made (the static rows make none)
    wgs = [dict(next=W, h=rnd.randrange(8), out=0, tag=[0] * ring, item=[NONE] * ring, read=[0] * ring)
           for _ in range(nwg)]

    def claim(S):  # WgQueue::publish's head loop
        while S["out"] < 8:
            j = heads[S["h"]]
            heads[S["h"]] += 1
            claims[0] += 1
            it = j * 8 + S["h"]
            if it < items:
                return it
            S["out"] += 1
            if S["out"] < 8:
                S["h"] = (S["h"] + 1) % 8
        return NONE

    waves = []
    for b in range(nwg):
        for w in range(W):
            waves.append(dict(wg=b, st="own", k=None, grp=b * W + w, done=False,
                              pub=LEAD if (w == 0 and own_rows == 1) else 0))
    active = list(waves)
    steps = 0
    while active:
        steps += 1
        assert steps < 200 * (ngroups + nwaves * (own_rows + 1)) + 10000, "a wait cycle"
        wv = rnd.choice(active)
        S = wgs[wv["wg"]]
        if wv["st"] == "own":  # a group in hand (row 0's, a static slot's or an item's)
            wv["st"] = "publish_then_work" if wv["pub"] else "work"
        if wv["st"] in ("publish_then_work", "publish_then_exit"):
            x = wv["pub"]
            e, pe = x % ring, (x - 1) % ring
            if x >= 2 and S["tag"][pe] != x - 1:
                continue  # spin: batch order
            if x > ring and S["read"][e] != W:
                continue  # spin: the entry's previous batch not read by all yet
            assert x <= ring or S["tag"][e] == x - ring
            it = claim(S)
            S["item"][e], S["read"][e], S["tag"][e] = it, 0, x
            wv["pub"] = 0
            if wv["st"] == "publish_then_exit":
                wv["done"] = True
                active.remove(wv)
                continue
            wv["st"] = "work"
            continue
        if wv["st"] == "work":
            if wv["grp"] < ngroups:
                seen[wv["grp"]] += 1
            k = S["next"]
            S["next"] += 1
            wv["k"] = k
            if k < own_rows * W:  # a static slot
                if k == (own_rows - 1) * W:
                    wv["pub"] = LEAD
                wv["grp"] = (k // W) * nwaves + W * wv["wg"] + k % W
                wv["st"] = "own"
                continue
            if k % W == 0:
                wv["pub"] = k // W - own_rows + 1 + LEAD
            wv["st"] = "read"
            continue
        if wv["st"] == "read":
            b, slot = wv["k"] // W - own_rows + 1, wv["k"] % W
            e = b % ring
            if S["tag"][e] != b:
                assert S["tag"][e] < b, "entry overwritten before it was read"
                continue  # spin
            it = S["item"][e]
            S["read"][e] += 1
            assert S["read"][e] <= W
            if it == NONE:
                if wv["pub"]:
                    wv["st"] = "publish_then_exit"
                else:
                    wv["done"] = True
                    active.remove(wv)
                continue
            wv["grp"] = own_groups + it * W + slot
            wv["st"] = "publish_then_work" if wv["pub"] else "work"
    assert all(wv["done"] for wv in waves)
    return seen, items, claims[0]


def _ngroups_cases(K0, nwaves, W):
    base = K0 * nwaves
    return sorted({max(base - 1, 0), base, base + 1,
                   base + 3 * W,          # a tail of fewer than 8 items (3)
                   base + 7 * W,          # 7 items
                   base + 5 * W + 1,      # the last item holds one group (W > 1: fewer than W)
                   base + 8 * 3 * W + 5,  # every head hands out three items, and a short last one
                   base + 11 * W - 1})


@pytest.mark.parametrize("K0", [1, 2, 5, "rows"])
@pytest.mark.parametrize("ring", [4, 2])
def test_every_group_once(K0, ring):
    for W, nwg in [(1, 1), (2, 3), (4, 8), (16, 2), (16, 24)]:
        nwaves = nwg * W
        if K0 == "rows":  # no queue items: the static rows cover the batch
            cases = [(rows, rows * nwaves - d) for rows in (1, 3, 6) for d in (0, 1, nwaves - 1) if rows * nwaves - d > 0]
        else:
            cases = [(K0, ng) for ng in _ngroups_cases(K0, nwaves, W)]
        for k0, ng in cases:
            for seed in range(6):
                seen, items, claims = simulate(ng, nwg, W, k0, ring, seed * 131 + ng)
                assert all(s == 1 for s in seen), (ng, nwg, W, k0, ring, seed)
                if K0 == "rows":
                    assert items == 0
                # every item claimed once, and each workgroup sees each head exhausted once
                assert claims == items + 8 * nwg


def test_own_rows_one_is_the_full_queue():
    """K0 = 1 against the full queue's restatement under the same interleaving
    (seed): both process the same groups, each once."""
    import test_queue_schedule as full
    for seed in range(40):
        r = random.Random(seed)
        W, nwg = r.choice([1, 2, 4, 16]), r.choice([1, 2, 8])
        ng = r.randrange(1, 3000)
        assert simulate(ng, nwg, W, 1, 4, seed)[0] == full.simulate(ng, nwg, W, 1, 4, seed)


def test_kernel_restated():
    """The kernel's slot arithmetic is the one simulated here."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "lsbm_amd", "csrc", "crc32c_kernels.hip")).read()
    assert re.search(r"k < own_rows \* kWavesPerWg", src)
    assert re.search(r"k == \(own_rows - 1\) \* kWavesPerWg\) pend_pub = kWqLead", src)
    assert re.search(r"bt = k / kWavesPerWg - own_rows \+ 1", src)
    assert re.search(r"grp = own_groups \+ \(uint64_t\)it \* kWavesPerWg \+ slot", src)
    units = open(os.path.join(root, "lsbm_amd", "csrc", "crc32c_units.h")).read()
    m = re.search(r"kWqRing = (\d+), kWqLead = (\d+)", units)
    assert m and (int(m.group(2)), int(m.group(1))) == (LEAD, 4)
