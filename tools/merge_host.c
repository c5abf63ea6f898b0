/* merge_host.c -- the host's compaction merge restated in C: a k-way
 * compare-and-advance merge in the shape of MergingIterator::FindSmallest
 * (table/merger.cc:155-168), the drop rule of DoCompactionWork
 * (lsbm/db_impl.cc:999-1032) and the copy of the kept keys -- the CPU figure
 * tools/bench_merge.py prints beside the GPU's plan + gather.  Arrays as
 * include/lsbm_merge.h takes them.  On one thread it is the reference's loop;
 * on T threads the key space is cut at T - 1 splitter keys (every run is
 * searched for each splitter, so equal keys stay in one part and the merge
 * stays stable), each thread merges its part, the drop rule is evaluated per
 * merged position from its predecessor, and the parts are compacted by a
 * prefix sum.  Built by the tool at run time:
 *     gcc -O2 -fPIC -shared -pthread -o build/libmergehost.so tools/merge_host.c
 */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MAX_RUNS 64
#define MAX_THREADS 64
#define MAX_SEQ ((1ull << 56) - 1)

typedef struct {
  const uint8_t* keys;
  const uint64_t* koff;
  const uint64_t* values;
  uint64_t n;
  const uint64_t* run_first;
  uint32_t n_runs;
  int internal, drop, bottom;
  uint64_t snapshot;
  uint64_t* order;   /* n: the merged order, before the drop */
  uint8_t* keep;     /* n */
  uint64_t* source;  /* outputs */
  uint8_t* out_keys;
  uint64_t* out_koff;
  uint64_t* out_values;
} shared_t;

typedef struct {
  shared_t* s;
  uint64_t lo[MAX_RUNS], hi[MAX_RUNS]; /* this part's slice of every run */
  uint64_t p0, p1;                     /* its merged positions */
  uint64_t kept, kept_bytes;           /* after pass 2; then the part's output base */
} job_t;

static int compare(const shared_t* s, uint64_t a, uint64_t b) {
  const uint8_t *ka = s->keys + s->koff[a], *kb = s->keys + s->koff[b];
  uint64_t la = s->koff[a + 1] - s->koff[a], lb = s->koff[b + 1] - s->koff[b];
  if (s->internal) {
    la -= 8;
    lb -= 8;
  }
  const uint64_t m = la < lb ? la : lb;
  int c = memcmp(ka, kb, m);
  if (c == 0) c = la < lb ? -1 : (la > lb ? 1 : 0);
  if (c == 0 && s->internal) {
    uint64_t ta, tb;
    memcpy(&ta, ka + la, 8);
    memcpy(&tb, kb + lb, 8);
    c = ta > tb ? -1 : (ta < tb ? 1 : 0);
  }
  return c;
}

/* first entry of [lo, hi) that is not below entry `key` */
static uint64_t lower_bound(const shared_t* s, uint64_t lo, uint64_t hi, uint64_t key) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (compare(s, mid, key) < 0) lo = mid + 1; else hi = mid;
  }
  return lo;
}

static void* merge_part(void* arg) {
  job_t* j = (job_t*)arg;
  const shared_t* s = j->s;
  uint64_t at[MAX_RUNS], p = j->p0;
  for (uint32_t r = 0; r < s->n_runs; r++) at[r] = j->lo[r];
  for (;;) { /* FindSmallest: the candidate changes only on a strict < */
    int smallest = -1;
    for (uint32_t r = 0; r < s->n_runs; r++)
      if (at[r] < j->hi[r] && (smallest < 0 || compare(s, at[r], at[smallest]) < 0)) smallest = (int)r;
    if (smallest < 0) break;
    s->order[p++] = at[smallest]++;
  }
  return 0;
}

static void* drop_part(void* arg) {
  job_t* j = (job_t*)arg;
  const shared_t* s = j->s;
  uint64_t kept = 0, bytes = 0;
  for (uint64_t p = j->p0; p < j->p1; p++) {
    const uint64_t e = s->order[p], len = s->koff[e + 1] - s->koff[e];
    int keep = 1;
    if (s->drop) {
      uint64_t tag;
      memcpy(&tag, s->keys + s->koff[e + 1] - 8, 8);
      if ((tag & 0xff) <= 1) {
        uint64_t last_seq = MAX_SEQ;
        if (p) {
          const uint64_t q = s->order[p - 1], qlen = s->koff[q + 1] - s->koff[q];
          uint64_t qtag;
          memcpy(&qtag, s->keys + s->koff[q + 1] - 8, 8);
          if ((qtag & 0xff) <= 1 && qlen == len && !memcmp(s->keys + s->koff[q], s->keys + s->koff[e], len - 8))
            last_seq = qtag >> 8;
        }
        if (last_seq <= s->snapshot || ((tag & 0xff) == 0 && (tag >> 8) <= s->snapshot && s->bottom)) keep = 0;
      }
    }
    s->keep[p] = (uint8_t)keep;
    if (keep) {
      kept++;
      bytes += len;
    }
  }
  j->kept = kept;
  j->kept_bytes = bytes;
  return 0;
}

static void* copy_part(void* arg) {
  job_t* j = (job_t*)arg;
  const shared_t* s = j->s;
  uint64_t o = j->kept, b = j->kept_bytes; /* (now the part's output base) */
  for (uint64_t p = j->p0; p < j->p1; p++) {
    if (!s->keep[p]) continue;
    const uint64_t e = s->order[p], len = s->koff[e + 1] - s->koff[e];
    s->source[o] = e;
    s->out_koff[o] = b;
    s->out_values[2 * o] = s->values[2 * e];
    s->out_values[2 * o + 1] = s->values[2 * e + 1];
    memcpy(s->out_keys + b, s->keys + s->koff[e], len);
    o++;
    b += len;
  }
  return 0;
}

static void run_all(void* (*fn)(void*), job_t* jobs, int t) {
  pthread_t th[MAX_THREADS];
  for (int i = 1; i < t; i++) pthread_create(&th[i], 0, fn, &jobs[i]);
  fn(&jobs[0]);
  for (int i = 1; i < t; i++) pthread_join(th[i], 0);
}

/* Returns 0; counts[0] = n_out, counts[1] = the output's key bytes.  order
 * (8 n bytes) and keep (n bytes) are the caller's scratch. */
int merge_host(const uint8_t* keys, const uint64_t* koff, const uint64_t* values, uint64_t n,
               const uint64_t* run_first, uint32_t n_runs, int internal, uint32_t flags, uint64_t snapshot,
               uint64_t* order, uint8_t* keep, uint64_t* source, uint8_t* out_keys, uint64_t* out_koff,
               uint64_t* out_values, uint64_t* counts, int threads) {
  if (n_runs > MAX_RUNS || threads < 1 || threads > MAX_THREADS) return 1;
  shared_t s = {keys, koff, values, n, run_first, n_runs, internal, (int)(flags & 1), (int)((flags >> 1) & 1),
                snapshot, order, keep, source, out_keys, out_koff, out_values};
  job_t* jobs = (job_t*)calloc((size_t)threads, sizeof(job_t));
  if (!jobs) return 1;
  /* the splitters come from the longest run */
  uint32_t longest = 0;
  for (uint32_t r = 1; r < n_runs; r++)
    if (run_first[r + 1] - run_first[r] > run_first[longest + 1] - run_first[longest]) longest = r;
  for (int t = 0; t < threads; t++) {
    jobs[t].s = &s;
    for (uint32_t r = 0; r < n_runs; r++) {
      uint64_t cut = run_first[r + 1];
      if (t + 1 < threads && n_runs) {
        const uint64_t len = run_first[longest + 1] - run_first[longest];
        const uint64_t at = run_first[longest] + len * (uint64_t)(t + 1) / (uint64_t)threads;
        cut = at < run_first[longest + 1] ? lower_bound(&s, run_first[r], run_first[r + 1], at) : run_first[r + 1];
      }
      jobs[t].hi[r] = cut;
      jobs[t].lo[r] = t ? jobs[t - 1].hi[r] : run_first[r];
    }
    jobs[t].p0 = t ? jobs[t - 1].p1 : 0;
    jobs[t].p1 = jobs[t].p0;
    for (uint32_t r = 0; r < n_runs; r++) jobs[t].p1 += jobs[t].hi[r] - jobs[t].lo[r];
  }
  run_all(merge_part, jobs, threads);
  run_all(drop_part, jobs, threads);
  uint64_t o = 0, b = 0;
  for (int t = 0; t < threads; t++) {
    const uint64_t k = jobs[t].kept, kb = jobs[t].kept_bytes;
    jobs[t].kept = o;
    jobs[t].kept_bytes = b;
    o += k;
    b += kb;
  }
  run_all(copy_part, jobs, threads);
  out_koff[o] = b;
  counts[0] = o;
  counts[1] = b;
  free(jobs);
  return 0;
}
