// memcut_kernels.hip -- gfx950 kernels of the memtable switch
// (include/lsbm_memtable_cut.h): the skiplist's heights and the arena's
// accounting, and with them where RecoverLogFile and MakeRoomForWrite end a
// memtable.
//
// Heights (three kernels).  The generator is x <- 16807 x mod (2^31 - 1), so
// the state before draw t is rnd * 16807^t: every lane jumps to its own 64
// draws.  What a range of draws does to `h = 1; while (h < 12 && Next() % 4 ==
// 0) h++` depends on the state it is entered with (successes so far, 0..10)
// only until its first failure, so a range is summed up as a McRun, and runs
// compose.  mc_heights_runs_kernel sums up each lane's 64 draws and each
// workgroup's 16,384; mc_heights_link_kernel walks the workgroups' runs with
// one lane (about n / 12,000 steps) and gives every workgroup the inserts
// before it and its entry state; mc_heights_emit_kernel walks the draws again
// and stores each insert's height and the generator state after it.  11 n
// draws always hold n inserts (the cap ends an insert after 11 successes),
// which sizes the grid; workgroups past the n-th insert leave at once.
//
// Cut (three kernels, the walk in two forms).  mc_slots_kernel checks the input and writes one word
// per slot: an entry's encoded length, or a record's test point.
// mc_walk_kernel is one workgroup, of which one wave walks.  The workgroup
// moves a chunk of 4,096 slot words into LDS with the heights the chunk can
// need (those that continue the memtable that enters it, and the table's
// first 4,096 for a memtable that begins in it), the wave walks the chunk out
// of LDS and leaves each slot's usage in place of its word, and the workgroup
// stores the chunk: the walk itself waits for no global load or store.  The
// wave takes 64 slots a step: each lane has its
// entry's cost roundup8(L) + 8 + 8 height, a wave scan gives the running cost,
// and every lane tests whether it is the first that is not a plain fit into
// the arena's current block (or a test point whose test is true, or a slot
// that finds no memtable).  A ballot finds that lane, its slot is resolved
// with the reference's allocator step by step, and the lanes behind it test
// again against the new state: one round per event, about one per 4,096 bytes,
// instead of one dependent step per entry.  Everything the walk decides goes
// to the scratch (mc_walk_lane_kernel is the same walk by one lane, slot by slot: the fallback it was measured
// against, chosen by LSBM_MEMCUT_WALK=lane); mc_commit_kernel copies it out only if the status is OK, so
// an error leaves the outputs as they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"  // wave_incl_scan
#include "memcut_types.h"

namespace lsbm {
namespace {

// a b mod 2^31 - 1 for a, b < 2^31 (util/random.h's reduction, folded twice)
__device__ __forceinline__ uint64_t mc_mul(uint64_t a, uint64_t b) {
  const uint64_t p = a * b;
  uint64_t r = (p & kMcM) + (p >> 31);
  r = (r & kMcM) + (r >> 31);
  return r >= kMcM ? r - kMcM : r;
}

__device__ __forceinline__ uint64_t mc_pow(uint64_t e) {  // 16807^e
  uint64_t r = 1, b = kMcA;
  for (; e; e >>= 1) {
    if (e & 1) r = mc_mul(r, b);
    b = mc_mul(b, b);
  }
  return r;
}

// the state before the first draw; a state no generator has (the cut refuses
// it) is made one, so that the arithmetic stays in range
__device__ __forceinline__ uint64_t mc_first_state(const McHeightsArgs& a) {
  const uint64_t x = (a.d_rnd ? a.d_rnd[0] : a.rnd) % kMcM;
  return x ? x : 1;
}

__device__ __forceinline__ McRun mc_lane_run(uint64_t x) {
  McRun r = {0, 0, 0, kMcDraws};
  bool failed = false;
  for (uint32_t i = 0; i < kMcDraws; i++) {
    x = mc_mul(x, kMcA);
    const bool ok = (x & 3) == 0;
    if (!failed) {
      if (ok) r.lead++;
      else failed = true;  // (this insert is counted where the run is applied)
    } else if (ok) {
      if (++r.tail == kMcMaxHeight - 1) r.rest++, r.tail = 0;
    } else {
      r.rest++, r.tail = 0;
    }
  }
  return r;
}

// the inserts a run completes when entered with s successes, and the state after it
__device__ __forceinline__ void mc_apply(const McRun& r, uint32_t s, uint64_t& done, uint32_t& s_out) {
  const uint32_t t = s + r.lead;
  if (r.lead == r.len) {
    done = t / (kMcMaxHeight - 1), s_out = t % (kMcMaxHeight - 1);
  } else {
    done = t / (kMcMaxHeight - 1) + 1 + r.rest, s_out = r.tail;
  }
}

__device__ __forceinline__ McRun mc_compose(const McRun& x, const McRun& y) {
  if (x.lead == x.len) return McRun{x.len + y.lead, y.rest, y.tail, x.len + y.len};
  uint64_t done;
  uint32_t s;
  mc_apply(y, x.tail, done, s);
  return McRun{x.lead, x.rest + (uint32_t)done, s, x.len + y.len};
}

__device__ __forceinline__ uint64_t mc_lane_state(const McHeightsArgs& a) {  // before this lane's draws
  const uint64_t at = ((uint64_t)blockIdx.x * kMcThreads + threadIdx.x) * kMcDraws;
  return mc_mul(mc_first_state(a), mc_pow(at));
}

__global__ __launch_bounds__(kMcThreads) void mc_heights_runs_kernel(McHeightsArgs a) {
  __shared__ McRun runs[kMcThreads];
  runs[threadIdx.x] = mc_lane_run(mc_lane_state(a));
  __syncthreads();
  if (threadIdx.x == 0) {
    McRun all = runs[0];
    for (uint32_t i = 1; i < kMcThreads; i++) all = mc_compose(all, runs[i]);
    a.runs[blockIdx.x] = all;
  }
}

__global__ __launch_bounds__(kMcThreads) void mc_heights_link_kernel(McHeightsArgs a) {
  for (uint64_t w = threadIdx.x; w < a.n_wgs; w += kMcThreads) a.link[2 * w] = a.n;  // nothing to emit
  __syncthreads();
  if (threadIdx.x) return;
  if (a.n == 0 && a.rnd_out) a.rnd_out[0] = mc_first_state(a);
  uint64_t before = 0;
  uint32_t s = 0;
  for (uint64_t w = 0; w < a.n_wgs && before < a.n; w++) {
    a.link[2 * w] = before, a.link[2 * w + 1] = s;
    uint64_t done;
    mc_apply(a.runs[w], s, done, s);
    before += done;
  }
}

struct McLaneStart {
  uint64_t before;
  uint32_t s, pad;
};

__global__ __launch_bounds__(kMcThreads) void mc_heights_emit_kernel(McHeightsArgs a) {
  __shared__ McRun runs[kMcThreads];
  __shared__ McLaneStart starts[kMcThreads];
  const uint64_t wg_before = a.link[2 * (uint64_t)blockIdx.x];
  if (wg_before >= a.n) return;
  uint64_t x = mc_lane_state(a);
  runs[threadIdx.x] = mc_lane_run(x);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t before = wg_before;
    uint32_t s = (uint32_t)a.link[2 * (uint64_t)blockIdx.x + 1];
    for (uint32_t i = 0; i < kMcThreads; i++) {
      starts[i].before = before, starts[i].s = s;
      uint64_t done;
      mc_apply(runs[i], s, done, s);
      before += done;
    }
  }
  __syncthreads();
  uint64_t e = starts[threadIdx.x].before;
  uint32_t s = starts[threadIdx.x].s;
  for (uint32_t i = 0; i < kMcDraws && e < a.n; i++) {
    x = mc_mul(x, kMcA);
    uint32_t h = 0;
    if ((x & 3) == 0) {
      if (++s == kMcMaxHeight - 1) h = kMcMaxHeight;  // the cap: the loop ends without a draw
    } else {
      h = s + 1;
    }
    if (h) {
      a.heights[e] = (uint8_t)h;
      if (a.rnd_after) a.rnd_after[e] = (uint32_t)x;
      if (e + 1 == a.n && a.rnd_out) a.rnd_out[0] = x;
      e++, s = 0;
    }
  }
}

// ---- cut ----

__device__ __forceinline__ uint64_t mc_varint_length(uint64_t v) {  // v < 2^32
  return 1 + (v >= (1u << 7)) + (v >= (1u << 14)) + (v >= (1u << 21)) + (v >= (1u << 28));
}

// the record whose slots hold slot s: the last i < n_records with entry_base[i] + i <= s
__device__ __forceinline__ uint64_t mc_record_of(const uint64_t* entry_base, uint64_t n_records, uint64_t s) {
  uint64_t lo = 0, hi = n_records;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (entry_base[mid] + mid <= s) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kMcThreads) void mc_slots_kernel(McCutArgs a) {
  const uint64_t items = a.n_slots > a.n_records + 1 ? a.n_slots : a.n_records + 1;
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * kMcThreads + threadIdx.x; i < items; i += (uint64_t)gridDim.x * kMcThreads) {
    if (i <= a.n_records) {
      const uint64_t b = a.entry_base[i];
      if (i == 0 && b != 0) bad = true;
      if (i == a.n_records && b != a.n_entries) bad = true;
      if (i < a.n_records && a.entry_base[i + 1] < b) bad = true;
    }
    if (i >= a.n_slots) continue;
    uint64_t word = kSlotDead << kSlotKindShift;
    if (a.n_records) {
      const uint64_t r = mc_record_of(a.entry_base, a.n_records, i);
      const uint64_t b0 = a.entry_base[r], b1 = a.entry_base[r + 1];
      const uint64_t k = i - (b0 + r), cnt = b1 >= b0 ? b1 - b0 : 0;
      const uint32_t st = a.mode == kMcRecover && a.rec_status ? a.rec_status[r] : 0;
      const bool skipped = st == 1 || st == 6 || st == 7;  // LSBM_WB_TOO_SMALL, _BAD_INPUT, _NO_ROOM
      const bool test = a.mode == kMcRecover ? k == cnt : k == 0;
      const uint64_t j = a.mode == kMcRecover ? k : k - 1;
      const uint64_t e = b0 + j;
      if (skipped) {
      } else if (test) {
        word = kSlotTest << kSlotKindShift;
      } else if (j < cnt && e < a.n_entries) {
        const uint64_t k0 = a.key_offsets[e], k1 = a.key_offsets[e + 1];
        const uint64_t ikl = k1 - k0 + a.key_extra;
        const uint32_t type = a.types ? a.types[e] : 1;
        const uint64_t vl = type == 0 ? 0 : a.values[2 * e + 1];
        if (k1 < k0 || ikl >> 32 || vl >> 32 || type > 1) {
          bad = true;
        } else {
          word = (mc_varint_length(ikl) + ikl + mc_varint_length(vl) + vl) | kSlotEntry << kSlotKindShift;
        }
      }
    }
    a.words[i] = word;
  }
  if (bad) *a.status = kMcBadInput;
}

__device__ __forceinline__ uint64_t mc_bcast(uint64_t v, uint32_t lane) {  // lane: the same in every lane
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, (int)lane);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)lane);
  return (uint64_t)hi << 32 | lo;
}

__device__ __forceinline__ uint64_t mc_usage(uint64_t blocks_memory, uint64_t n_blocks) {
  // the blocks and the capacity of the vector that holds them: the least power of two >= n_blocks
  const uint64_t cap = n_blocks <= 1 ? 1 : 1ull << (64 - __builtin_clzll(n_blocks - 1));
  return blocks_memory + 8 * cap;
}

__device__ __forceinline__ uint64_t mc_cost(uint64_t word, uint32_t h) {
  const uint64_t L = word & ((1ull << kSlotKindShift) - 1);
  return (word >> kSlotKindShift) == kSlotEntry ? ((L + 7) & ~7ull) + 8 + 8 * h : 0;
}

// kLane: the fallback the wave's arrangement is measured against.  The staging is the same; lane 0 alone walks
// the chunk slot by slot, with the host loop's shortcut for an entry that fits.
template <bool kLane>
__device__ __forceinline__ void mc_walk(const McCutArgs& a) {
  // a chunk of slots: the words, overwritten in place by the usage after each slot
  __shared__ uint64_t s_words[kMcChunk];
  __shared__ uint8_t s_hc[kMcChunk];  // the heights of the memtable that enters the chunk, from its next insert on
  __shared__ uint8_t s_h0[kMcChunk];  // the heights of a memtable that begins in the chunk: the table's first ones
  __shared__ int64_t s_j;             // this memtable's inserts in this call before the chunk
  __shared__ uint32_t s_from_state;
  const uint32_t lane = threadIdx.x;  // (of wave 0: the other waves only move chunks)
  if (*a.status != kMcOk) return;
  uint64_t have = 0, rem = 0, nb = 0, bm = 0, rnd_in = kMcSeed, ein = 0;
  if (a.state_in) {
    have = a.state_in[0], rem = a.state_in[1], nb = a.state_in[2], bm = a.state_in[3], rnd_in = a.state_in[4];
    ein = a.state_in[5];
    if (have > 1 || rem > kMcBlock || (rem & 7) || (have && nb == 0) || rnd_in == 0 || rnd_in >= kMcM) {
      if (threadIdx.x == 0) *a.status = kMcBadInput;
      return;
    }
  }
  const uint64_t wbs = a.write_buffer_size;
  bool have_mem = have != 0, pending = have_mem, from_state = have_mem;
  uint64_t U = have_mem ? mc_usage(bm, nb) : 0;  // ApproximateMemoryUsage(), 0 without a memtable
  int64_t R0 = (int64_t)rem;   // a lane's entry is a plain fit while its running cost is <= R0
  int64_t jstep = 0;           // this memtable's inserts in this call before the step's first lane
  int64_t estep = (int64_t)ein;  // and over all calls
  uint64_t m = 0, continues = 0;
  const uint64_t below = (1ull << (lane & 63)) - 1;

  for (uint32_t i = threadIdx.x; i < kMcChunk; i += kMcThreads) s_h0[i] = i < a.n_entries ? a.h0[i] : 0;
  if (threadIdx.x == 0) s_j = 0, s_from_state = from_state;
  __syncthreads();
  for (uint64_t cbase = 0; cbase < a.n_slots; cbase += kMcChunk) {
    {
      const uint8_t* H = s_from_state ? a.h1 : a.h0;
      const uint64_t j0 = (uint64_t)s_j;
      for (uint32_t i = threadIdx.x; i < kMcChunk; i += kMcThreads) {
        s_words[i] = cbase + i < a.n_slots ? a.words[cbase + i] : 0;
        s_hc[i] = j0 + i < a.n_entries ? H[j0 + i] : 0;
      }
    }
    __syncthreads();
    if (kLane && threadIdx.x == 0) {
      const int64_t jchunk = jstep;
      bool created_in_chunk = false;
      uint64_t r = (uint64_t)R0;
      const uint64_t left = a.n_slots - cbase;
      const uint32_t cnt = (uint32_t)(left < kMcChunk ? left : kMcChunk);
      for (uint32_t i = 0; i < cnt; i++) {
        const uint64_t w = s_words[i], kind = w >> kSlotKindShift;
        if (kind == kSlotDead) {
          s_words[i] = U;
          continue;
        }
        if (kind == kSlotTest && a.mode == kMcWrite && have_mem && U > wbs) {
          if (pending) pending = false;
          else a.mem_use[m++] = U;
          have_mem = false;
        }
        if (!have_mem) {
          a.mem_slot[m] = cbase + i;
          have_mem = true, pending = false, from_state = false, created_in_chunk = true;
          bm = kMcBlock, nb = 1, r = kMcBlock - kMcHeadNode, U = kMcFresh, jstep = 0, estep = 0;
        } else if (pending) {
          a.mem_slot[0] = cbase + i;
          pending = false, continues = 1;
        }
        if (kind == kSlotEntry) {
          const uint64_t L = w & ((1ull << kSlotKindShift) - 1);
          const uint64_t node = 8 + 8 * (uint64_t)(created_in_chunk ? s_h0[jstep] : s_hc[jstep - jchunk]);
          const uint64_t cost = ((L + 7) & ~7ull) + node;
          if (cost <= r) {
            r -= cost;
          } else {
            if (L <= r) r -= L;
            else if (L > kMcBlock / 4) bm += L, nb++;
            else bm += kMcBlock, nb++, r = kMcBlock - L;
            const uint64_t slop = r & 7;
            if (node + slop <= r) r -= node + slop;
            else bm += kMcBlock, nb++, r = kMcBlock - node;
            U = mc_usage(bm, nb);
          }
          jstep++, estep++;
        }
        s_words[i] = U;
        if (kind == kSlotTest && a.mode == kMcRecover && U > wbs) {
          a.mem_use[m++] = U;
          have_mem = false, U = 0;
        }
      }
      R0 = (int64_t)r;
      s_j = jstep, s_from_state = from_state;
    }
    if (!kLane && threadIdx.x < kMcWave) {
      const int64_t jchunk = jstep;
      bool created_in_chunk = false;
      const uint64_t left = a.n_slots - cbase;
      const uint32_t steps = (uint32_t)((left < kMcChunk ? left : kMcChunk) + kMcWave - 1) / kMcWave;
      for (uint32_t st = 0; st < steps; st++) {
    const uint64_t base = cbase + st * kMcWave;
    const uint64_t w_cur = s_words[st * kMcWave + lane];
    const uint64_t kind = w_cur >> kSlotKindShift;
    const bool entry = kind == kSlotEntry, test = kind == kSlotTest, live = kind != kSlotDead;
    const uint64_t emask = __ballot(entry);
    const int64_t pfx = __popcll(emask & below), tot = __popcll(emask);
    uint32_t h = 0;
    if (entry) h = created_in_chunk ? s_h0[jstep + pfx] : s_hc[jstep - jchunk + pfx];
    uint64_t c = mc_cost(w_cur, h);
    uint64_t S = wave_incl_scan(c, lane);
    uint64_t my_usage = U;
    for (uint32_t start = 0; start < kMcWave;) {
      const bool ev = live && lane >= start &&
                      (!have_mem || pending || (test && U > wbs) || (entry && (int64_t)S > R0));
      const uint64_t mask = __ballot(ev);
      if (!mask) {
        if (lane >= start) my_usage = U;
        break;
      }
      const uint32_t f = __builtin_ctzll(mask);
      if (lane >= start && lane < f) my_usage = U;
      const uint64_t wf = mc_bcast(w_cur, f);
      const uint64_t kf = wf >> kSlotKindShift;
      const int64_t pf = (int64_t)mc_bcast((uint64_t)pfx, f);
      uint64_t r = (uint64_t)(R0 - (int64_t)mc_bcast(S - c, f));  // the block's bytes left before this slot
      // MakeRoomForWrite's test comes before the record
      if (kf == kSlotTest && a.mode == kMcWrite && have_mem && U > wbs) {
        if (pending) pending = false;  // (the state's memtable ends without a record of this call)
        else {
          if (lane == 0) a.mem_use[m] = U;
          m++;
        }
        have_mem = false;
      }
      if (!have_mem) {  // new MemTable: the arena's first block holds the skiplist's head
        if (lane == 0) a.mem_slot[m] = base + f;
        have_mem = true, pending = false, from_state = false, created_in_chunk = true;
        bm = kMcBlock, nb = 1, r = kMcBlock - kMcHeadNode, U = kMcFresh;
        jstep = -pf, estep = -pf;
        if (entry && lane >= f) h = s_h0[pfx - pf];
        c = mc_cost(w_cur, h);
        S = wave_incl_scan(c, lane);
      } else if (pending) {  // the state's memtable takes this call's first record
        if (lane == 0) a.mem_slot[0] = base + f;
        pending = false, continues = 1;
      }
      if (kf == kSlotEntry) {
        const uint64_t L = wf & ((1ull << kSlotKindShift) - 1);
        const uint64_t node = 8 + 8 * (uint64_t)__builtin_amdgcn_readlane((int)h, (int)f);
        // Arena::Allocate(L)
        if (L <= r) r -= L;
        else if (L > kMcBlock / 4) bm += L, nb++;
        else bm += kMcBlock, nb++, r = kMcBlock - L;
        // Arena::AllocateAligned(node)
        const uint64_t slop = r & 7;
        if (node + slop <= r) r -= node + slop;
        else bm += kMcBlock, nb++, r = kMcBlock - node;
        U = mc_usage(bm, nb);
      }
      if (lane == f) my_usage = U;
      if (kf == kSlotTest && a.mode == kMcRecover && U > wbs) {  // RecoverLogFile's test follows the record
        if (lane == 0) a.mem_use[m] = U;
        m++;
        have_mem = false, U = 0;
      }
      R0 = (int64_t)r + (int64_t)mc_bcast(S, f);
      start = f + 1;
    }
    R0 -= (int64_t)mc_bcast(S, kMcWave - 1);
    jstep += tot, estep += tot;
    s_words[st * kMcWave + lane] = my_usage;
      }
      if (lane == 0) s_j = jstep, s_from_state = from_state;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kMcChunk && cbase + i < a.n_slots; i += kMcThreads)
      a.uout[cbase + i] = s_words[i];
    __syncthreads();
  }

  if (threadIdx.x) return;
  const bool open = have_mem && !pending;
  const uint64_t n_mem = m + (open ? 1 : 0);
  if (open) a.mem_use[m] = U;
  uint64_t rnd = kMcSeed;
  if (have_mem) {
    if (jstep > 0) rnd = (from_state ? a.r1 : a.r0)[jstep - 1];
    else rnd = from_state ? rnd_in : kMcSeed;
  }
  uint64_t* out = a.hdr + kMcState;
  out[0] = have_mem, out[1] = have_mem ? (uint64_t)R0 : 0, out[2] = have_mem ? nb : 0, out[3] = have_mem ? bm : 0;
  out[4] = rnd, out[5] = have_mem ? (uint64_t)estep : 0;
  a.hdr[kMcMems] = n_mem, a.hdr[kMcContinues] = continues;
  if (n_mem > a.mem_cap) *a.status = kMcNoRoom;
}

__global__ __launch_bounds__(kMcThreads) void mc_walk_kernel(McCutArgs a) { mc_walk<false>(a); }
__global__ __launch_bounds__(kMcThreads) void mc_walk_lane_kernel(McCutArgs a) { mc_walk<true>(a); }

__global__ __launch_bounds__(kMcThreads) void mc_commit_kernel(McCutArgs a) {
  if (*a.status != kMcOk) return;
  const uint64_t n_mem = a.hdr[kMcMems];
  const uint64_t items = a.n_records > n_mem + 1 ? a.n_records : n_mem + 1;
  for (uint64_t i = (uint64_t)blockIdx.x * kMcThreads + threadIdx.x; i < items; i += (uint64_t)gridDim.x * kMcThreads) {
    if (i < a.n_records) a.usage[i] = a.uout[a.entry_base[i + 1] + i];  // the record's last slot
    if (i < n_mem) {
      a.mem_first[i] = mc_record_of(a.entry_base, a.n_records, a.mem_slot[i]);
      a.mem_usage[i] = a.mem_use[i];
    }
    if (i == n_mem) a.mem_first[i] = a.n_records;
    if (i == 0) {
      a.counts[0] = n_mem, a.counts[1] = a.hdr[kMcContinues];
      for (uint32_t k = 0; k < 6; k++) a.state_out[k] = a.hdr[kMcState + k];
    }
  }
}

}  // namespace

hipError_t launch_heights(const McHeightsArgs& a, hipStream_t stream) {
  const dim3 block(kMcThreads), grid((uint32_t)a.n_wgs);
  hipLaunchKernelGGL(mc_heights_runs_kernel, grid, block, 0, stream, a);
  hipLaunchKernelGGL(mc_heights_link_kernel, dim3(1), block, 0, stream, a);
  hipLaunchKernelGGL(mc_heights_emit_kernel, grid, block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_memcut(const McCutArgs& a, int lane_grid, hipStream_t stream) {
  const dim3 block(kMcThreads);
  hipLaunchKernelGGL(mc_slots_kernel, dim3(lane_grid), block, 0, stream, a);
  if (a.one_lane) hipLaunchKernelGGL(mc_walk_lane_kernel, dim3(1), block, 0, stream, a);
  else hipLaunchKernelGGL(mc_walk_kernel, dim3(1), block, 0, stream, a);
  hipLaunchKernelGGL(mc_commit_kernel, dim3(lane_grid), block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace lsbm
