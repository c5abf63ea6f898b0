// table_pack_kernels.hip -- gfx950 kernels of the table packer
// (include/lsbm_table_pack.h): TableBuilder::WriteBlock's keep rule with the
// file offsets that follow from it (table/table_builder.cc:176-206), and the
// mover that puts every block, raw or compressed, at its final offset.
//
// pack_plan_tile_kernel   one lane per block: the rule, the size that is kept,
//                         and size + gap scanned over the tile of kPackThreads
//                         blocks; the tile's total.
// pack_scan_tiles_kernel  one workgroup: running sums over the tiles' totals
//                         (shared by plan and mover), the grand total.
// pack_plan_apply_kernel  one lane per block: its tile's running sum and
//                         first_offset added to its offset.
// pack_count_kernel       one lane per block: the range checks and the status,
//                         and its number of pieces scanned over the tile.
// pack_move_kernel        a piece is 4 KiB of one block's destination, cut at
//                         16-byte boundaries of the destination's address.  A
//                         wave takes 64 pieces: each lane looks one up, then
//                         the wave moves them one after the other, every lane
//                         busy: a lane stores aligned 16-byte chunks, each
//                         made of the two aligned 16-byte source words it
//                         straddles, shifted by the wave-uniform difference of
//                         the two phases.  A block's first and last partial
//                         chunk, and a chunk whose source words would reach
//                         outside the source image, go byte by byte.
//
// A piece finds its block by a binary search over the running sums of the
// pieces.  What is read back from scratch is not trusted: the mover checks the
// block it found again (ranges, type, piece number) before it moves a byte.
// Every loop halves a range or advances.  No spin-waits, no cross-workgroup
// state inside a launch, no LDS in the mover.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"  // gcu8, gu8, u32x4, gcu32x4, gu32x4, block_excl_sum
#include "table_pack_types.h"

namespace lsbm {
namespace {

// ---------------------------------------------------------------- plan

__global__ __launch_bounds__(kPackThreads) void pack_plan_tile_kernel(PackPlanArgs a) {
  __shared__ uint64_t lds[kPackWaves];
  const uint64_t i = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
  uint64_t size = 0, v = 0;
  uint32_t type = 0;
  if (i < a.n) {
    const uint64_t raw = a.raw_len[i];
    const uint64_t comp = a.comp_len ? a.comp_len[i] : UINT64_MAX;
    // compressed.size() < raw.size() - raw.size() / 8 (table/table_builder.cc:187)
    type = (comp != UINT64_MAX && comp < raw - raw / 8) ? 1u : 0u;
    size = type ? comp : raw;
    v = size + a.gap;
  }
  uint64_t excl, total;
  block_excl_sum<kPackWaves>(v, lds, excl, total);
  if (i < a.n) {
    a.types[i] = (uint8_t)type;
    a.handles[2 * i] = excl;
    a.handles[2 * i + 1] = size;
  }
  if (threadIdx.x == 0) a.tiles[blockIdx.x] = total;
}

// tiles[t] becomes the sum of the tiles before t, tiles[n_tiles] the sum of all
__global__ __launch_bounds__(kPackThreads) void pack_scan_tiles_kernel(uint64_t* tiles, uint64_t n_tiles,
                                                                        uint64_t* end, uint64_t first_offset) {
  __shared__ uint64_t lds[kPackWaves];
  uint64_t carry = 0;
  for (uint64_t base = 0; base < n_tiles; base += kPackThreads) {
    const uint64_t t = base + threadIdx.x;
    uint64_t excl, total;
    block_excl_sum<kPackWaves>(t < n_tiles ? tiles[t] : 0, lds, excl, total);
    if (t < n_tiles) tiles[t] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) {
    tiles[n_tiles] = carry;
    if (end) end[0] = first_offset + carry;
  }
}

__global__ __launch_bounds__(kPackThreads) void pack_plan_apply_kernel(PackPlanArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
  if (i < a.n) a.handles[2 * i] += a.first_offset + a.tiles[blockIdx.x];
}

// ---------------------------------------------------------------- pack

struct PackBlock {
  uint64_t dst;      // address of the block's first destination byte
  uint64_t src;      // address of its first source byte
  uint64_t img_lo;   // the source image, as addresses
  uint64_t img_hi;
  uint64_t size;
  uint32_t status;
};

// block i with every range checked; dst / src are meaningful with status kPackOk
__device__ __forceinline__ PackBlock pack_block(const PackArgs& a, uint64_t i) {
  PackBlock b = {};
  const uint64_t off = a.handles[2 * i], size = a.handles[2 * i + 1];
  const uint32_t type = a.types[i];
  uint32_t st = kPackOk;
  if (off > a.out_size || size > a.out_size - off || a.gap > a.out_size - off - size) st = kPackNoRoom;
  const uint8_t* img = nullptr;
  uint64_t img_size = 0, so = 0;
  if (type == 0) {
    img = a.raw;
    img_size = a.raw_size;
    if (a.raw_handles) so = a.raw_handles[2 * i]; else st = kPackBadInput;
  } else if (type == 1) {
    img = a.comp;
    img_size = a.comp_size;
    if (a.comp_offsets) so = a.comp_offsets[i]; else st = kPackBadInput;
  } else {
    st = kPackBadInput;
  }
  if (so > img_size || size > img_size - so) st = kPackBadInput;
  b.status = st;
  b.size = size;
  b.dst = reinterpret_cast<uint64_t>(a.out) + off;
  b.img_lo = reinterpret_cast<uint64_t>(img);
  b.img_hi = b.img_lo + img_size;
  b.src = b.img_lo + so;
  return b;
}

// chunks: the aligned 16-byte units of the destination that hold a byte of the block
__device__ __forceinline__ uint64_t pack_chunks(const PackBlock& b) {
  return b.size ? ((b.dst & (kPackChunk - 1)) + b.size + kPackChunk - 1) / kPackChunk : 0;
}

// pieces of kPackPieceChunks chunks; the last one takes up to one chunk more
__device__ __forceinline__ uint64_t pack_pieces(uint64_t chunks) {
  return chunks <= kPackPieceChunks + 1 ? (chunks ? 1 : 0) : (chunks + kPackPieceChunks - 2) / kPackPieceChunks;
}

__global__ __launch_bounds__(kPackThreads) void pack_count_kernel(PackArgs a) {
  __shared__ uint64_t lds[kPackWaves];
  const uint64_t i = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
  uint64_t pieces = 0;
  if (i < a.n) {
    const PackBlock b = pack_block(a, i);
    a.status[i] = b.status;
    if (b.status == kPackOk) pieces = pack_pieces(pack_chunks(b));
  }
  uint64_t excl, total;
  block_excl_sum<kPackWaves>(pieces, lds, excl, total);
  if (i < a.n) a.pieces[i] = excl;
  if (threadIdx.x == 0) a.tiles[blockIdx.x] = total;
}

// the pieces of the blocks before block i (i < n)
__device__ __forceinline__ uint64_t pieces_before(const PackArgs& a, uint64_t i) {
  return a.pieces[i] + a.tiles[i / kPackThreads];
}

// dword j of the 128-bit window that starts `bits` bits into {v[j], v[j+1]}
__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t bits) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> bits);
}

// chunks a lane has in flight: a piece is two rounds of 2 x 64 lanes x 16 bytes.
// (4 in flight measured slower: 131 registers, 3 waves a SIMD, against 96 and 5.)
constexpr int kPackUnroll = 2;

__device__ __forceinline__ uint64_t lane_value(uint64_t v, uint32_t j) {  // (j wave-uniform)
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)j);
  return ((uint64_t)hi << 32) | lo;
}

// What a piece needs, looked up by one lane: the block it belongs to (checked
// again), the piece's chunks [c0, c0 + count) and which image the block is from.
struct PackPiece {
  uint64_t dst, src, size, c0;
  uint32_t count;  // 0: nothing to move
  uint32_t type;
};

__device__ __forceinline__ PackPiece find_piece(const PackArgs& a, uint64_t piece, uint64_t total) {
  PackPiece r = {};
  // the block of this piece: the last i with pieces_before(i) <= piece.  With
  // blocks of one piece each that is block `piece` itself: tried first.
  uint64_t lo = 0, hi = a.n;
  if (piece < a.n && pieces_before(a, piece) == piece &&
      (piece + 1 == a.n ? total : pieces_before(a, piece + 1)) > piece)
    lo = piece, hi = piece + 1;
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (pieces_before(a, mid) <= piece) lo = mid; else hi = mid;
  }
  const uint64_t first = pieces_before(a, lo);
  if (first > piece) return r;  // (not a scan of these blocks)
  const PackBlock b = pack_block(a, lo);
  const uint64_t chunks = pack_chunks(b), p = piece - first, pieces = pack_pieces(chunks);
  if (b.status != kPackOk || p >= pieces) return r;
  r.dst = b.dst;
  r.src = b.src;
  r.size = b.size;
  r.c0 = p * kPackPieceChunks;
  r.count = (uint32_t)((p + 1 == pieces ? chunks : r.c0 + kPackPieceChunks) - r.c0);  // <= kPackPieceChunks + 1
  r.type = a.types[lo];
  return r;
}

__global__ __launch_bounds__(kPackThreads) void pack_move_kernel(PackArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t total = a.tiles[a.n_tiles];
  const uint64_t stride = (uint64_t)gridDim.x * kPackWaves * 64;
  // a wave takes 64 consecutive pieces: every lane looks one up (the dependent
  // reads of 64 lookups overlap), then the wave moves them one after the other
  for (uint64_t first = ((uint64_t)blockIdx.x * kPackWaves + (threadIdx.x >> 6)) * 64; first < total;
       first += stride) {
    PackPiece mine = {};
    if (first + lane < total) mine = find_piece(a, first + lane, total);
    const uint32_t cnt = __builtin_amdgcn_readfirstlane((uint32_t)(total - first < 64 ? total - first : 64));
    for (uint32_t j = 0; j < cnt; j++) {
      const uint32_t count = (uint32_t)__builtin_amdgcn_readlane((int)mine.count, (int)j);
      if (count == 0) continue;
      const uint32_t type = (uint32_t)__builtin_amdgcn_readlane((int)mine.type, (int)j);
      const uint64_t dst = lane_value(mine.dst, j), src = lane_value(mine.src, j);
      const uint64_t end = dst + lane_value(mine.size, j), c0 = lane_value(mine.c0, j), c1 = c0 + count;
      const uint64_t img_lo = reinterpret_cast<uint64_t>(type ? a.comp : a.raw);
      const uint64_t img_hi = img_lo + (type ? a.comp_size : a.raw_size);
      const uint64_t aligned = dst & ~(uint64_t)(kPackChunk - 1);
      // the source address of an aligned destination chunk, and its phase (the same for every chunk)
      const uint64_t delta = src - dst;
      const uint32_t sh = (uint32_t)(delta & (kPackChunk - 1)), q = sh >> 2, bits = (sh & 3) * 8;
      const uint32_t need = sh ? 2 * kPackChunk : kPackChunk;  // the source bytes a chunk is made of
      for (uint64_t base = c0; base < c1; base += 64 * kPackUnroll) {
        // wide: the chunk's aligned source words are inside the image (they may
        // reach past the block's own bytes: the head's and the tail's do)
        bool in[kPackUnroll], wide[kPackUnroll];
        // chunk k of this lane: its destination, and the aligned source word that holds its first byte
        const uint64_t d0 = aligned + (base + lane) * kPackChunk, s0 = d0 + delta - sh;
#define PACK_D(k) (d0 + (uint64_t)(k) * (64 * kPackChunk))
#define PACK_S(k) (s0 + (uint64_t)(k) * (64 * kPackChunk))
#pragma unroll
        for (int k = 0; k < kPackUnroll; k++) {
          in[k] = base + (uint64_t)k * 64 + lane < c1;
          wide[k] = in[k] && PACK_S(k) >= img_lo && PACK_S(k) + need <= img_hi;
        }
        const uint64_t some = __ballot(wide[0]);
        if (some) {  // (wave-uniform; a piece without it is a few bytes at the edge of an image)
          // every load is issued before the first is used, none under a branch:
          // a lane without a wide chunk reads some lane's, and stores nothing
          const uint64_t spare = lane_value(s0, (uint32_t)__builtin_ctzll(some));
          u32x4 x[kPackUnroll], y[kPackUnroll];
#pragma unroll
          for (int k = 0; k < kPackUnroll; k++) x[k] = *reinterpret_cast<gcu32x4>(wide[k] ? PACK_S(k) : spare);
          if (sh) {
#pragma unroll
            for (int k = 0; k < kPackUnroll; k++) y[k] = *reinterpret_cast<gcu32x4>((wide[k] ? PACK_S(k) : spare) + kPackChunk);
          } else {
#pragma unroll
            for (int k = 0; k < kPackUnroll; k++) y[k] = x[k];
          }
#pragma unroll
          for (int k = 0; k < kPackUnroll; k++) {
            uint32_t v0, v1, v2, v3, v4;
            switch (q) {  // (wave-uniform)
              case 0: v0 = x[k].x, v1 = x[k].y, v2 = x[k].z, v3 = x[k].w, v4 = y[k].x; break;
              case 1: v0 = x[k].y, v1 = x[k].z, v2 = x[k].w, v3 = y[k].x, v4 = y[k].y; break;
              case 2: v0 = x[k].z, v1 = x[k].w, v2 = y[k].x, v3 = y[k].y, v4 = y[k].z; break;
              default: v0 = x[k].w, v1 = y[k].x, v2 = y[k].y, v3 = y[k].z, v4 = y[k].w; break;
            }
            const u32x4 r = {funnel(v0, v1, bits), funnel(v1, v2, bits), funnel(v2, v3, bits), funnel(v3, v4, bits)};
            if (wide[k]) {
              if (PACK_D(k) >= dst && PACK_D(k) + kPackChunk <= end) {
                *reinterpret_cast<gu32x4>(PACK_D(k)) = r;
              } else {  // the block's head or tail: its bytes one at a time, out of the registers
                const uint64_t lo = PACK_D(k) > dst ? PACK_D(k) : dst, hi = PACK_D(k) + kPackChunk < end ? PACK_D(k) + kPackChunk : end;
                const uint64_t r0 = ((uint64_t)r.y << 32) | r.x, r1 = ((uint64_t)r.w << 32) | r.z;
#pragma unroll 1
                for (uint64_t t = lo; t < hi; t++) {
                  const uint32_t i = (uint32_t)(t - PACK_D(k));
                  *reinterpret_cast<gu8>(t) = (uint8_t)((i < 8 ? r0 : r1) >> (8 * (i & 7)));
                }
              }
            }
          }
        }
#pragma unroll
        for (int k = 0; k < kPackUnroll; k++) {
          if (in[k] && !(some && wide[k])) {  // at the edge of the source image: byte by byte
            const uint64_t lo = PACK_D(k) > dst ? PACK_D(k) : dst, hi = PACK_D(k) + kPackChunk < end ? PACK_D(k) + kPackChunk : end;
#pragma unroll 1
            for (uint64_t t = lo; t < hi; t++) *reinterpret_cast<gu8>(t) = *reinterpret_cast<gcu8>(t + delta);
          }
        }
#undef PACK_D
#undef PACK_S
      }
    }
  }
}

}  // namespace

hipError_t launch_pack_plan(const PackPlanArgs& a, hipStream_t stream) {
  const dim3 grid((uint32_t)a.n_tiles), block(kPackThreads);
  if (a.n) hipLaunchKernelGGL(pack_plan_tile_kernel, grid, block, 0, stream, a);
  hipLaunchKernelGGL(pack_scan_tiles_kernel, dim3(1), block, 0, stream, a.tiles, a.n_tiles, a.end, a.first_offset);
  if (a.n) hipLaunchKernelGGL(pack_plan_apply_kernel, grid, block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_pack(const PackArgs& a, hipStream_t stream) {
  if (!a.n) return hipSuccess;
  const dim3 grid((uint32_t)a.n_tiles), block(kPackThreads);
  hipLaunchKernelGGL(pack_count_kernel, grid, block, 0, stream, a);
  hipLaunchKernelGGL(pack_scan_tiles_kernel, dim3(1), block, 0, stream, a.tiles, a.n_tiles, (uint64_t*)nullptr,
                     (uint64_t)0);
  // a wave per 64 pieces; valid blocks that do not overlap have at most n + out_size / 4 KiB pieces
  uint64_t wgs = ((a.n + a.out_size / (kPackChunk * kPackPieceChunks)) / 64 + kPackWaves) / kPackWaves;
  if (wgs > kPackMaxGrid) wgs = kPackMaxGrid;
  hipLaunchKernelGGL(pack_move_kernel, dim3((uint32_t)wgs), block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace lsbm
