/* block_build_host.c -- the host's BlockBuilder::Add / Finish loop
 * (table/block_builder.cc:57-107) restated in C, on T threads: the CPU figure
 * tools/bench_block_build.py prints beside the GPU's block_build.  Entries,
 * block_first and windows as include/lsbm_block_build.h takes them; every
 * window must hold its block (the tool sizes them from the plan).  Built by
 * the tool at run time:
 *     gcc -O2 -fPIC -shared -pthread -o build/libblockbuild.so tools/block_build_host.c
 */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  const uint8_t* keys;
  const uint64_t* key_offsets;
  const uint64_t* values;
  const uint8_t* image;
  const uint64_t* block_first;
  uint32_t interval;
  uint8_t* out;
  const uint64_t* handles;
  uint64_t* built;
  uint64_t b0, b1;
} job_t;

static uint8_t* put_varint32(uint8_t* p, uint32_t v) {
  while (v >= 128) {
    *p++ = (uint8_t)(v | 128);
    v >>= 7;
  }
  *p++ = (uint8_t)v;
  return p;
}

static uint64_t build_block(const job_t* j, uint64_t b) {
  uint8_t* const dst = j->out + j->handles[2 * b];
  uint8_t* p = dst;
  const uint64_t e0 = j->block_first[b], e1 = j->block_first[b + 1];
  const uint64_t cap = (e1 - e0) / j->interval + 2;
  uint32_t stack[512];
  uint32_t* restarts = cap <= 512 ? stack : (uint32_t*)malloc(cap * sizeof(uint32_t));
  uint32_t nr = 1, counter = 0;
  restarts[0] = 0;
  const uint8_t* last = 0;
  uint64_t last_len = 0;
  for (uint64_t e = e0; e < e1; e++) {
    const uint8_t* key = j->keys + j->key_offsets[e];
    const uint64_t klen = j->key_offsets[e + 1] - j->key_offsets[e], vlen = j->values[2 * e + 1];
    uint64_t shared = 0;
    if (counter < j->interval) {
      const uint64_t m = last_len < klen ? last_len : klen;
      while (shared < m && last[shared] == key[shared]) shared++;
    } else {
      restarts[nr++] = (uint32_t)(p - dst);
      counter = 0;
    }
    p = put_varint32(p, (uint32_t)shared);
    p = put_varint32(p, (uint32_t)(klen - shared));
    p = put_varint32(p, (uint32_t)vlen);
    memcpy(p, key + shared, klen - shared);
    p += klen - shared;
    memcpy(p, j->image + j->values[2 * e], vlen);
    p += vlen;
    last = key;
    last_len = klen;
    counter++;
  }
  memcpy(p, restarts, 4 * (size_t)nr);  /* EncodeFixed32 on a little-endian host */
  p += 4 * (size_t)nr;
  memcpy(p, &nr, 4);
  p += 4;
  if (restarts != stack) free(restarts);
  return (uint64_t)(p - dst);
}

static void* run(void* arg) {
  job_t* j = (job_t*)arg;
  for (uint64_t b = j->b0; b < j->b1; b++) j->built[b] = build_block(j, b);
  return 0;
}

int block_build_host(const uint8_t* keys, const uint64_t* key_offsets, const uint64_t* values, const uint8_t* image,
                     const uint64_t* block_first, uint64_t n_blocks, uint32_t interval, uint8_t* out,
                     const uint64_t* handles, uint64_t* built, int threads) {
  if (threads < 1) threads = 1;
  if (threads > 256) threads = 256;
  if (interval < 1) return -1;
  pthread_t th[256];
  job_t jobs[256];
  for (int t = 0; t < threads; t++) {
    job_t j = {keys, key_offsets, values, image, block_first, interval, out, handles, built,
               n_blocks * t / threads, n_blocks * (t + 1) / threads};
    jobs[t] = j;
    if (pthread_create(&th[t], 0, run, &jobs[t])) return -1;
  }
  for (int t = 0; t < threads; t++) pthread_join(th[t], 0);
  return 0;
}
