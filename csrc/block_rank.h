// Stable ranking steps shared by the selection, sort and partition kernels
// (kernels.hip compaction, join.hip direct-address probe, sort.hip,
// partition.hip, topk.hip).  They all split n rows into block-owned chunks,
// walk a chunk in tiles, and give every selected row an output slot that
// keeps row order:
//   slot = the block's running base            (rows of earlier tiles)
//        + rows of earlier waves of the tile   (wave totals through LDS)
//        + rows of earlier lanes of the wave   (ballot rank)
// The kernels stay separate; only these steps are written once.  Barriers
// belong to the caller unless a step says otherwise.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"

// ---------------------------------------------------------------------------
// host: block b owns rows [b * chunk, (b + 1) * chunk)
// ---------------------------------------------------------------------------

struct BlockChunks {
  int64_t chunk;
  int nblocks;
};

// chunk = max(ceil(n / kMaxBlocks), min_chunk) rounded up to multiple_of.
// A chunk is at least min_chunk rows so that small inputs do not spread over
// blocks with nearly nothing to do.
static inline BlockChunks block_chunks(int64_t n, int64_t min_chunk,
                                       int64_t multiple_of = 1) {
  int64_t chunk = std::max((n + kMaxBlocks - 1) / kMaxBlocks, min_chunk);
  chunk = (chunk + multiple_of - 1) / multiple_of * multiple_of;
  return {chunk, (int)((n + chunk - 1) / chunk)};
}

// ---------------------------------------------------------------------------
// device: one wave
// ---------------------------------------------------------------------------

DEV_INLINE int lane_id() { return threadIdx.x & (WAVE - 1); }
DEV_INLINE int wave_id() { return threadIdx.x / WAVE; }
// bits of the lanes below the caller
DEV_INLINE uint64_t lane_lt_mask() { return (1ull << lane_id()) - 1; }

// Rank of the caller among the lanes of its wave that have sel set;
// *wave_total is how many there are.  Every lane of the wave must call it
// (ballots are wave-wide).
DEV_INLINE int wave_rank(bool sel, int* wave_total) {
  uint64_t ballot = __ballot(sel);
  *wave_total = __popcll(ballot);
  return __popcll(ballot & lane_lt_mask());
}

// Lanes of this wave that are active and hold the same digit d as the
// caller; `bits` ballot rounds tell 2^bits digits apart.  Every lane of the
// wave must call it.
DEV_INLINE uint64_t wave_peers(int d, bool active, int bits) {
  uint64_t peers = __ballot(active);
  for (int b = 0; b < bits; ++b) {
    bool bit = (d >> b) & 1;
    uint64_t vote = __ballot(bit);
    peers &= bit ? vote : ~vote;
  }
  return peers;
}

// ---------------------------------------------------------------------------
// device: across the waves of a block
// ---------------------------------------------------------------------------

// Sum of v over the block: a wave reduce, then one LDS atomic per wave.
// Thread 0 gets the total (so does every other thread).  Holds two
// barriers; every thread of the block must call it.
DEV_INLINE int32_t block_sum(int32_t v) {
  __shared__ int32_t acc;
  if (threadIdx.x == 0) acc = 0;
  __syncthreads();
  for (int off = WAVE / 2; off; off >>= 1) v += __shfl_down(v, off, WAVE);
  if (lane_id() == 0) atomicAdd(&acc, v);
  __syncthreads();
  return acc;
}

// The cross-wave step of a compaction tile, in two halves with the caller's
// barrier between them: each wave puts its total into an LDS row of NWAVES
// cells, then every thread reads the row.  `before` is the total of the
// earlier waves and `total` that of the tile; all threads see the same
// `total`, so each can keep the block's running base in a register.
DEV_INLINE void wave_total_put(int32_t* row, int32_t wave_total) {
  if (lane_id() == 0) row[wave_id()] = wave_total;
}

struct WaveSpan {
  int32_t before, total;
};

template <int NWAVES>
DEV_INLINE WaveSpan wave_span(const int32_t* row) {
  const int wid = wave_id();
  WaveSpan s{0, 0};
#pragma unroll
  for (int w = 0; w < NWAVES; ++w) {
    int32_t c = row[w];
    s.before += w < wid ? c : 0;
    s.total += c;
  }
  return s;
}

// ---------------------------------------------------------------------------
// device: stable digit scatter of one tile
// ---------------------------------------------------------------------------
// running[d] is the block's next free output position for digit d and
// wave_hist[w][d] the rows of wave w in this tile with digit d; nbins <= BINS
// digits are in use.  A row's position is running[d] + rows of earlier
// waves with digit d + its rank among its wave's peers.  Per tile, every
// thread of the block calls digit_tile_begin, loads its row, calls
// digit_tile_pos, stores at the returned position, and calls
// digit_tile_end.  The four barriers of a tile are inside the calls: one at
// the end of begin, one in pos, two around the sums of end.

template <int BINS, int NWAVES>
DEV_INLINE void digit_tile_begin(int nbins, int32_t (*wave_hist)[BINS]) {
  for (int b = threadIdx.x; b < nbins; b += blockDim.x)
    for (int w = 0; w < NWAVES; ++w) wave_hist[w][b] = 0;
  __syncthreads();
}

template <int BINS, typename Pos>
DEV_INLINE Pos digit_tile_pos(int d, bool active, int bits,
                              const Pos* running,
                              int32_t (*wave_hist)[BINS]) {
  const int wid = wave_id();
  uint64_t peers = wave_peers(d, active, bits);
  int rank_in_wave = __popcll(peers & lane_lt_mask());
  if (active && rank_in_wave == 0) wave_hist[wid][d] = __popcll(peers);
  __syncthreads();
  if (!active) return 0;
  int32_t before = 0;
  for (int w = 0; w < wid; ++w) before += wave_hist[w][d];
  return running[d] + before + rank_in_wave;
}

template <int BINS, int NWAVES, typename Pos>
DEV_INLINE void digit_tile_end(int nbins, Pos* running,
                               const int32_t (*wave_hist)[BINS]) {
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += blockDim.x) {
    int32_t t = 0;
    for (int w = 0; w < NWAVES; ++w) t += wave_hist[w][b];
    running[b] += t;
  }
  __syncthreads();
}
