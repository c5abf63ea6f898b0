"""Pure-Python model of the memtable switch (include/lsbm_memtable_cut.h):
MemTable::ApproximateMemoryUsage() after every record, and where
DBImpl::RecoverLogFile and DBImpl::MakeRoomForWrite end a memtable.

    heights(rnd, n)                     RandomHeight() of n inserts, the state after
    entry_size(ikl, vl)                 MemTable::Add's encoded length
    Arena                               util/arena.cc's counters
    cut(entries, entry_base, ...)       lsbm_memtable_cut_dev's outputs

An entry is (internal key length, value length, type); a state is the list
{have_mem, remaining, n_blocks, blocks_memory, rnd, entries_in_mem}.
"""
M = 2147483647
A = 16807
SEED = 0xdeadbeef & 0x7fffffff
MAX_HEIGHT = 12
BRANCHING = 4
BLOCK = 4096
FRESH_USAGE = 4104
RECOVER, WRITE = 0, 1
OK, NO_ROOM, BAD_INPUT = 0, 1, 2
WB_SKIPPED = (1, 6, 7)  # LSBM_WB_TOO_SMALL, _BAD_INPUT, _NO_ROOM
NO_STATE = [0, 0, 0, 0, SEED, 0]


def varint_length(v):
    n = 1
    while v >= 128:
        v >>= 7
        n += 1
    return n


def entry_size(ikl, vl):
    return varint_length(ikl) + ikl + varint_length(vl) + vl


def random_height(rnd):
    """(height, the generator's state after it)."""
    h = 1
    while h < MAX_HEIGHT:
        rnd = rnd * A % M
        if rnd % BRANCHING:
            break
        h += 1
    return h, rnd


def heights(rnd, n):
    out = []
    for _ in range(n):
        h, rnd = random_height(rnd)
        out.append(h)
    return out, rnd


def cap_of(n_blocks):
    """std::vector's capacity after n_blocks push_backs (libstdc++ doubles)."""
    c = 1
    while c < n_blocks:
        c *= 2
    return c


class Arena:
    def __init__(self, remaining=0, n_blocks=0, blocks_memory=0):
        self.remaining, self.n_blocks, self.blocks_memory = remaining, n_blocks, blocks_memory

    def _fallback(self, b):
        self.n_blocks += 1
        if b > BLOCK // 4:
            self.blocks_memory += b
        else:
            self.blocks_memory += BLOCK
            self.remaining = BLOCK - b

    def allocate(self, b):
        if b <= self.remaining:
            self.remaining -= b
        else:
            self._fallback(b)

    def allocate_aligned(self, b):
        needed = b + self.remaining % 8
        if needed <= self.remaining:
            self.remaining -= needed
        else:
            self._fallback(b)

    def usage(self):
        return self.blocks_memory + 8 * cap_of(self.n_blocks)


def state_fault(st):
    have, rem, nb, _, rnd, _ = st
    return have > 1 or rem > BLOCK or rem % 8 or (have and nb == 0) or rnd == 0 or rnd >= M


def cut(entries, entry_base, rec_status=None, mode=RECOVER, write_buffer_size=4 << 20, state=None, mem_cap=None):
    """dict(status, usage, mem_first, mem_usage, counts, state), or
    dict(status) on an error."""
    n_records = len(entry_base) - 1
    if write_buffer_size < FRESH_USAGE or n_records < 0 or entry_base[0] != 0 or entry_base[-1] != len(entries) or \
            any(entry_base[i] > entry_base[i + 1] for i in range(n_records)):
        return dict(status=BAD_INPUT)
    st = list(state) if state is not None else list(NO_STATE)
    if state_fault(st):
        return dict(status=BAD_INPUT)
    have, arena, rnd, count = bool(st[0]), Arena(st[1], st[2], st[3]), st[4], st[5]
    last = arena.usage() if have else 0
    listed = False  # the current memtable has taken a record of this call
    pending = have  # it is the state's, and no record has reached it yet
    usage, mem_first, mem_usage, continues = [], [], [], 0

    def end():
        nonlocal have, listed, pending, last
        if listed:
            mem_usage.append(last)
        have = listed = pending = False
        last = 0

    def begin(i):
        nonlocal have, listed, pending, arena, rnd, count, last, continues
        if not have:
            arena, rnd, count = Arena(), SEED, 0
            arena.allocate_aligned(8 + 8 * MAX_HEIGHT)
            have, last = True, arena.usage()
        elif pending:
            continues, pending = 1, False
        if not listed:
            mem_first.append(i)
            listed = True

    for i in range(n_records):
        if mode == RECOVER and rec_status is not None and rec_status[i] in WB_SKIPPED:
            usage.append(last)
            continue
        if mode == WRITE and have and last > write_buffer_size:
            end()
        begin(i)
        for ikl, vl, t in entries[entry_base[i]:entry_base[i + 1]]:
            if t > 1 or ikl >> 32 or (t == 1 and vl >> 32):
                return dict(status=BAD_INPUT)
            arena.allocate(entry_size(ikl, vl if t else 0))
            h, rnd = random_height(rnd)
            arena.allocate_aligned(8 + 8 * h)
            count += 1
        last = arena.usage()
        usage.append(last)
        if mode == RECOVER and last > write_buffer_size:
            end()
    if have and listed:
        mem_usage.append(last)
    if mem_cap is not None and len(mem_first) > mem_cap:
        return dict(status=NO_ROOM)
    out = [1, arena.remaining, arena.n_blocks, arena.blocks_memory, rnd, count] if have else list(NO_STATE)
    return dict(status=OK, usage=usage, mem_first=mem_first + [n_records], mem_usage=mem_usage,
                counts=[len(mem_first), continues], state=out)
