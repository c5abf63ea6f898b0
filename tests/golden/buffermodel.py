"""Plain-Python restatement of the part of lsbm's read path that is LSbM rather
than LevelDB: Builder::SaveTo on an empty base (lsbm/version_set.cc:1686-1770)
with Version::NewSortedTable (:312-346), and Version::Get over the sorted-table
lists (:349-623), line by line, with the Get / SkipFilterGet modes, over
getmodel's table reads -- the model the GPU's buffered Get (include/lsbm_probe.h,
lsbm_amd/buffered.py) is compared with.  tests/test_buffered.py pins it to the
reference's own results (tests/golden/buffered_fixture.json, buffered_tables.bin).

Beside the literal model stands the rule the device runs, as a second small
function: slots() lays out the sorted tables the walk can reach, candidate()
is what a slot offers a key, plan() picks a key's probes from the candidates,
rule_get() reads them in order.  test_buffered.py holds the two equal on
random trees.
"""
from golden import blockmodel as bm
from golden import getmodel as gm
from golden.blockmodel import INTERNAL_KEY

kNumLevels = 4
DELETION_PART, INSERTION_PART, COMPACTION_BUFFER, WARMINGUP_BUFFER = 0, 1, 2, 3
SLOT_LEVEL0, SLOT_WB, SLOT_DEL, SLOT_HEAD, SLOT_REST, SLOT_INS = range(6)
CAND_NONE, CAND_MISS, CAND_MAY, CAND_ERR = range(4)


class FileMeta:
    """FileMetaData: number, file_size, smallest, largest, visible."""

    def __init__(self, number, file_size, smallest, largest, visible=True):
        self.number, self.file_size = number, file_size
        self.smallest, self.largest, self.visible = bytes(smallest), bytes(largest), visible


class SortedTable:
    def __init__(self):
        self.next = self.prev = None
        self.files_ = []


class Params:
    """runtime::compaction_buffer_use_length, config::buffered_merge, runtime::read_cursor_key_."""

    def __init__(self, use_length=(0, 0, 0, 0), buffered_merge=False, read_cursor_keys=(b"", b"", b"", b"")):
        self.use_length = [int(u) for u in use_length]
        self.buffered_merge = bool(buffered_merge)
        self.read_cursor_keys = [bytes(k) for k in read_cursor_keys]


class ModelVersion:
    """Version: levels_[level][type], each the head of a circular list."""

    def __init__(self, compaction_buffer_length=(0, 20, 20, 3)):
        self.compaction_buffer_length = list(compaction_buffer_length)
        self.levels_ = [[None] * 4 for _ in range(kNumLevels)]
        for kind in range(4):
            for level in range(kNumLevels):
                self.new_sorted_table(level, kind)

    def new_sorted_table(self, level, kind):
        """Version::NewSortedTable (:312-346)."""
        head = SortedTable()
        if self.levels_[level][kind] is None:
            head.next = head
            head.prev = head
            self.levels_[level][kind] = head
        else:
            head.prev = self.levels_[level][kind].prev
            head.next = self.levels_[level][kind]
            head.prev.next = head
            head.next.prev = head
            self.levels_[level][kind] = head
        if kind == COMPACTION_BUFFER:
            listlength = 0
            head = self.levels_[level][kind]
            cur = head
            while True:
                listlength += 1
                cur = cur.next
                if not (cur is not head and listlength <= self.compaction_buffer_length[level]):
                    break
            while cur is not head:  # detach all after
                nxt = cur.next
                cur.prev.next = cur.next
                cur.next.prev = cur.prev
                cur = nxt

    def lists(self):
        """{(level, type): [[FileMeta]]}: every list from its head in ->next order."""
        out = {}
        for level in range(kNumLevels):
            for kind in range(4):
                head = self.levels_[level][kind]
                tables, cur = [], head
                while True:
                    tables.append(cur.files_)
                    cur = cur.next
                    if cur is head:
                        break
                out[(level, kind)] = tables
        return out

    def numbers(self):
        return {k: [[f.number for f in t] for t in v] for k, v in self.lists().items()}

    @classmethod
    def from_lists(cls, lists):
        """A version with the given lists ([[FileMeta]] per (level, type), head
        first), whatever SaveTo would have made of them."""
        v = cls()
        for (level, kind), tables in lists.items():
            nodes = [SortedTable() for _ in tables]
            for i, (node, files) in enumerate(zip(nodes, tables)):
                node.files_ = list(files)
                node.next = nodes[(i + 1) % len(nodes)]
                node.prev = nodes[i - 1]
            v.levels_[level][kind] = nodes[0]
        return v


def save_to(added, compaction_buffer_length=(0, 20, 20, 3)):
    """Builder::SaveTo (:1686-1770) into a new Version, the base being empty.
    added: {(level, type): [(FileMeta, live)]} in added order, live being
    MaybeAddFile's test (:1795)."""
    v = ModelVersion(compaction_buffer_length)
    for level in range(kNumLevels):
        for kind in range(4):
            # (the base's lists hold one empty table each: the loop at :1698 does not run)
            if kind in (COMPACTION_BUFFER, WARMINGUP_BUFFER) and len(v.levels_[level][kind].files_) != 0:  # :1725
                v.new_sorted_table(level, kind)
            files = added.get((level, kind), [])
            pre_largest = None
            for i in range(len(files)):
                f, live = files[i]
                if level > 0 and i > 0 and bm.compare(f.smallest, pre_largest, INTERNAL_KEY) < 0:  # :1743
                    v.new_sorted_table(level, kind)
                pre_largest = f.largest
                if live:
                    v.levels_[level][kind].files_.append(f)
            if kind in (COMPACTION_BUFFER, WARMINGUP_BUFFER) and len(v.levels_[level][kind].files_) != 0:  # :1765
                v.new_sorted_table(level, kind)
    return v


# ---------------------------------------------------------------- the table cache


def contain_key(table, ikey):
    """Table::ContainKey (table/table.cc:370-390)."""
    idx = bm.seek(table["index"], ikey, INTERNAL_KEY, value_is_handle=True)
    if idx["state"] == gm.BAD_HANDLE:  # Valid(), and DecodeFrom fails: no filter test
        return True
    if idx["state"] != gm.VALID:
        return False
    if table["filter"] is not None and not gm.filter_block_may_match(table["filter"], idx["handle"][0], ikey[:-8],
                                                                     table["bits_per_key"]):
        return False
    return True


def skip_filter_get(table, ikey, uncompress, verify):
    """Table::SkipFilterGet (table/table.cc:392-416): (state, found key, value)."""
    return gm.table_get(dict(table, filter=None), ikey, uncompress, verify, prechecked=False)


def _find(files, ikey):
    return gm.find_file([f.largest for f in files], ikey)


# ---------------------------------------------------------------- Version::Get, literally


def version_get(v, tables, p, user_key, sequence, uncompress=None, verify=True):
    """Version::Get (:349-623): (verdict, value or None, the FileMeta that
    decided or None).  tables: {number: getmodel.open_table result}."""
    user_key = bytes(user_key)
    ikey = gm.lookup_key(user_key, sequence)
    levels_ = v.levels_

    def search(files, skip_numbers):
        for f in files:
            if f.number not in skip_numbers:
                state, found, value = gm.table_get(tables[f.number], ikey, uncompress, verify)
            else:
                state, found, value = skip_filter_get(tables[f.number], ikey, uncompress, verify)
            verdict, value = gm.save_value(state, found, value, user_key)  # if (!s.ok()) return s; the switch
            if verdict != gm.UNDECIDED:
                return verdict, value, f
        return None

    # level 0
    files = []
    for f in levels_[0][DELETION_PART].files_:
        if f is not None and user_key >= f.smallest[:-8] and user_key <= f.largest[:-8]:
            files.append(f)
    if files:
        files.sort(key=lambda f: -f.number)  # NewestFirst
    ins0 = levels_[0][INSERTION_PART].files_
    index = _find(ins0, ikey)
    if index < len(ins0) and user_key >= ins0[index].smallest[:-8]:
        files.append(ins0[index])
    got = search(files, ())
    if got:
        return got

    def walk(head, limit, tablechecked, out):
        cur = head
        while True:
            if tablechecked > limit:
                break
            tablechecked += 1
            index = _find(cur.files_, ikey)
            if index < len(cur.files_):
                f = cur.files_[index]
                if f.visible and user_key >= f.smallest[:-8]:
                    out.append(f)
            cur = cur.next
            if cur is head:
                break

    for level in range(1, kNumLevels):
        use = p.use_length
        checkwb = p.buffered_merge and user_key > p.read_cursor_keys[level] and level > 1 and use[level - 1] > 0
        dele = levels_[level][DELETION_PART]
        ins = levels_[level][INSERTION_PART]
        cb = levels_[level][COMPACTION_BUFFER].next
        wb = levels_[level][WARMINGUP_BUFFER].next
        files = []
        index_del = _find(dele.files_, ikey)
        covered_by_del = use[level] == 0 and index_del < len(dele.files_) and \
            user_key >= dele.files_[index_del].smallest[:-8]
        if covered_by_del and contain_key(tables[dele.files_[index_del].number], ikey):
            if checkwb:
                walk(wb, use[level - 1], 0, files)
            del_file_num = dele.files_[index_del].number
            files.append(dele.files_[index_del])
            got = search(files, (del_file_num,))
            if got:
                return got
        files = []
        index_ins = _find(ins.files_, ikey)
        covered_by_ins = index_ins < len(ins.files_) and user_key >= ins.files_[index_ins].smallest[:-8] and \
            contain_key(tables[ins.files_[index_ins].number], ikey)
        if covered_by_ins:
            ins_file_number = ins.files_[index_ins].number
            head_file_number = 0
            if not covered_by_del:
                head = cb
                covered_by_head = False
                index_head = 0
                if use[level] > 0 and len(head.files_) > 0:
                    index_head = _find(head.files_, ikey)
                    covered_by_head = index_head < len(head.files_) and \
                        user_key >= head.files_[index_head].smallest[:-8] and \
                        contain_key(tables[head.files_[index_head].number], ikey)
                if use[level] == 0 or covered_by_head:
                    if checkwb:
                        walk(wb, use[level - 1], 0, files)
                if covered_by_head:
                    files.append(head.files_[index_head])
                    head_file_number = head.files_[index_head].number
            # checking the rest compaction buffer: cur = cb->next, the counter starts at 2
            cur = cb.next
            tablechecked = 2
            while True:
                if tablechecked > use[level]:
                    break
                tablechecked += 1
                index = _find(cur.files_, ikey)
                if index < len(cur.files_):
                    f = cur.files_[index]
                    if f.visible and user_key >= f.smallest[:-8]:
                        files.append(f)
                cur = cur.next
                if cur is cb:
                    break
            files.append(ins.files_[index_ins])
            got = search(files, (ins_file_number, head_file_number))
            if got:
                return got
    return gm.UNDECIDED, None, None


# ---------------------------------------------------------------- the rule the device runs


def slots(v, p):
    """[(level, kind, [FileMeta], level0)]: the sorted tables the walk can reach, in order."""
    out = []
    for f in sorted(v.levels_[0][DELETION_PART].files_, key=lambda f: -f.number):
        out.append((0, SLOT_LEVEL0, [f], True))
    out.append((0, SLOT_LEVEL0, v.levels_[0][INSERTION_PART].files_, False))
    use = p.use_length
    for level in range(1, kNumLevels):
        if p.buffered_merge and level > 1 and use[level - 1] > 0:
            wb = cur = v.levels_[level][WARMINGUP_BUFFER].next
            for _ in range(use[level - 1] + 1):
                out.append((level, SLOT_WB, cur.files_, False))
                cur = cur.next
                if cur is wb:
                    break
        out.append((level, SLOT_DEL, v.levels_[level][DELETION_PART].files_, False))
        cb = v.levels_[level][COMPACTION_BUFFER].next
        if use[level] > 0 and cb.files_:
            out.append((level, SLOT_HEAD, cb.files_, False))
        cur = cb.next
        for _ in range(max(use[level] - 1, 0)):
            out.append((level, SLOT_REST, cur.files_, False))
            cur = cur.next
            if cur is cb:
                break
        out.append((level, SLOT_INS, v.levels_[level][INSERTION_PART].files_, False))
    return out


def candidate(slot, tables, ikey, memo=None):
    """(code, FileMeta or None): what a slot offers a key.  memo: a dict that
    keeps a file's answer to a key (the same file sits in many slots)."""
    level, kind, files, level0 = slot
    user = ikey[:-8]
    f = None
    if level0:
        if files and files[0].smallest[:-8] <= user <= files[0].largest[:-8]:
            f = files[0]
    else:
        i = _find(files, ikey)
        if i < len(files) and user >= files[i].smallest[:-8] and (files[i].visible or kind not in (SLOT_WB, SLOT_REST)):
            f = files[i]
    if f is None:
        return CAND_NONE, None
    if memo is not None:
        if (f.number, ikey) not in memo:
            memo[(f.number, ikey)] = _code(tables[f.number], ikey)
        return memo[(f.number, ikey)], f
    return _code(tables[f.number], ikey), f


def _code(table, ikey):
    user = ikey[:-8]
    idx = bm.seek(table["index"], ikey, INTERNAL_KEY, value_is_handle=True)
    if idx["state"] in (gm.BAD_ENTRY, gm.BAD_CONTENTS):
        return CAND_ERR
    if idx["state"] == gm.BAD_HANDLE:
        return CAND_MAY
    if idx["state"] != gm.VALID:
        return CAND_MISS
    if table["filter"] is not None and not gm.filter_block_may_match(table["filter"], idx["handle"][0], user,
                                                                     table["bits_per_key"]):
        return CAND_MISS
    return CAND_MAY


def plan(kinds, cand, use_length, wb_enabled, cursor_keys, user_key):
    """The probes of one key: slot indices in order.  kinds: [(level, kind)]
    per slot; cand: the candidate code per slot (include/lsbm_probe.h)."""
    probes = []
    reads = lambda c: c in (CAND_MAY, CAND_ERR)
    for s, (level, kind) in enumerate(kinds):
        if level == 0 and reads(cand[s]):
            probes.append(s)
    for level in range(1, kNumLevels):
        mine = [s for s, (lv, _) in enumerate(kinds) if lv == level]
        if not mine:
            continue
        of = lambda k: [s for s in mine if kinds[s][1] == k]
        one = lambda k: cand[of(k)[0]] if of(k) else CAND_NONE
        use = use_length[level]
        checkwb = bool(wb_enabled[level]) and bytes(user_key) > bytes(cursor_keys[level])
        covered_by_del = use == 0 and one(SLOT_DEL) != CAND_NONE
        wbs = [s for s in of(SLOT_WB) if reads(cand[s])]
        if covered_by_del and one(SLOT_DEL) == CAND_MAY:
            if checkwb:
                probes += wbs
            probes += of(SLOT_DEL)
        if one(SLOT_INS) == CAND_MAY:
            if not covered_by_del:
                head_ok = use > 0 and one(SLOT_HEAD) == CAND_MAY
                if (use == 0 or head_ok) and checkwb:
                    probes += wbs
                if head_ok:
                    probes += of(SLOT_HEAD)
            probes += [s for s in of(SLOT_REST) if reads(cand[s])]
            probes += of(SLOT_INS)
    return probes


def wb_enabled(p):
    return [int(p.buffered_merge and level > 1 and p.use_length[level - 1] > 0) for level in range(kNumLevels)]


def rule_get(v, tables, p, user_key, sequence, uncompress=None, verify=True, layout=None, memo=None):
    """The device's route: (verdict, value, the FileMeta that decided, its slot
    or -1, the number of table reads, the number of probes planned)."""
    user_key = bytes(user_key)
    ikey = gm.lookup_key(user_key, sequence)
    layout = slots(v, p) if layout is None else layout
    cands = [candidate(s, tables, ikey, memo) for s in layout]
    probes = plan([(s[0], s[1]) for s in layout], [c for c, _ in cands], p.use_length, wb_enabled(p),
                  p.read_cursor_keys, user_key)
    for j, s in enumerate(probes):
        f = cands[s][1]
        if memo is None or ("read", f.number, ikey) not in memo:
            state, found, value = skip_filter_get(tables[f.number], ikey, uncompress, verify)
            read = gm.save_value(state, found, value, user_key)
            if memo is not None:
                memo[("read", f.number, ikey)] = read
        else:
            read = memo[("read", f.number, ikey)]
        verdict, value = read
        if verdict != gm.UNDECIDED:
            return verdict, value, f, s, j + 1, len(probes)
    return gm.UNDECIDED, None, None, -1, len(probes), len(probes)
