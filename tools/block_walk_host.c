/* block_walk_host.c -- the host's forward walk over SSTable blocks
 * (table/block.cc's SeekToFirst / Next loop, as tools/db_check_gpu.cc
 * --filters parses blocks), on T threads: the CPU figure tools/bench_block.py
 * prints beside the GPU's block_scan.  Built by the tool at run time:
 *     gcc -O2 -fPIC -shared -pthread -o build/libblockwalk.so tools/block_walk_host.c
 */
#include <pthread.h>
#include <stdint.h>
#include <string.h>

typedef struct {
  const uint8_t* image;
  const uint64_t* handles;
  uint64_t b0, b1;
  uint64_t entries, key_bytes, value_bytes, bad;
} job_t;

static const uint8_t* varint32(const uint8_t* p, const uint8_t* limit, uint32_t* v) {
  uint32_t r = 0;
  for (uint32_t shift = 0; shift <= 28 && p < limit; shift += 7) {
    uint32_t byte = *p++;
    if (byte & 128) {
      r |= (byte & 127) << shift;
    } else {
      *v = r | (byte << shift);
      return p;
    }
  }
  return 0;
}

static void walk_block(const uint8_t* d, uint64_t size, job_t* j) {
  uint32_t nr;
  if (size < 4) { j->bad++; return; }
  memcpy(&nr, d + size - 4, 4);
  if (nr > (size - 4) / 4) { j->bad++; return; }
  if (nr == 0) return;
  const uint8_t* limit = d + size - 4 * (1 + (uint64_t)nr);
  uint32_t r0;
  memcpy(&r0, limit, 4);
  const uint8_t* p = d + r0;
  uint64_t klen = 0;
  while (p < limit) {
    uint32_t sh, ns, vl;
    if (limit - p < 3) { j->bad++; return; }
    sh = p[0]; ns = p[1]; vl = p[2];
    if ((sh | ns | vl) < 128) {
      p += 3;
    } else if (!(p = varint32(p, limit, &sh)) || !(p = varint32(p, limit, &ns)) ||
               !(p = varint32(p, limit, &vl))) {
      j->bad++;
      return;
    }
    if ((uint64_t)(limit - p) < (uint64_t)ns + vl || klen < sh) { j->bad++; return; }
    klen = (uint64_t)sh + ns;
    j->entries++;
    j->key_bytes += klen;
    j->value_bytes += vl;
    p += ns + vl;
  }
}

static void* run(void* arg) {
  job_t* j = (job_t*)arg;
  for (uint64_t b = j->b0; b < j->b1; b++) walk_block(j->image + j->handles[2 * b], j->handles[2 * b + 1], j);
  return 0;
}

/* out: {entries, key bytes, value bytes, bad blocks}; handles must lie inside the image */
int block_walk_host(const uint8_t* image, const uint64_t* handles, uint64_t n, int threads, uint64_t* out) {
  if (threads < 1) threads = 1;
  if (threads > 256) threads = 256;
  pthread_t th[256];
  job_t jobs[256];
  for (int t = 0; t < threads; t++) {
    memset(&jobs[t], 0, sizeof(job_t));
    jobs[t].image = image;
    jobs[t].handles = handles;
    jobs[t].b0 = n * t / threads;
    jobs[t].b1 = n * (t + 1) / threads;
    if (pthread_create(&th[t], 0, run, &jobs[t])) return -1;
  }
  out[0] = out[1] = out[2] = out[3] = 0;
  for (int t = 0; t < threads; t++) {
    pthread_join(th[t], 0);
    out[0] += jobs[t].entries;
    out[1] += jobs[t].key_bytes;
    out[2] += jobs[t].value_bytes;
    out[3] += jobs[t].bad;
  }
  return 0;
}
