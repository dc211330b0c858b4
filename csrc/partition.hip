// Stable one-pass hash partitioner (gfx950): groups rows into P <= 256
// partitions by `hash % P` with one histogram kernel and one scatter kernel.
// That is a single radix digit, so it follows radix_hist_kernel /
// radix_scatter_kernel in sort.hip (same block decomposition, same ballot
// ranking) with these differences:
//   - the partition id is computed in registers in both kernels and never
//     written to memory;
//   - the scatter reads only the hashes and writes only perm[pos] = row
//     (8 B out per row; the sort scatter moves a 16 B key/value pair);
//   - the intra-wave ranking takes ceil(log2(P)) ballot rounds, not 8;
//   - block offsets and the running position are int64 end to end, so the
//     row count is not capped at 2^31 as it is in the sort.
// Used by the grace hash join, RepartitionOp and the RCCL exchange through
// rowops.hash_partition.
#include "common.h"
#include "host_args.h"
#include "api.h"

constexpr int PART_MAX = 256;
constexpr int PART_BLOCK = 256;
constexpr int PART_NWAVES = PART_BLOCK / WAVE;

// how the kernels turn a hash into a partition id (uniform across the grid)
struct PartSpec {
  uint32_t p;        // number of partitions, 1..256
  uint32_t two32;    // 2^32 mod p
  int bits;          // ceil(log2(p)): ballot rounds that tell ids apart
  bool pow2;
  bool remix;
};

// h % p in unsigned 64-bit arithmetic.  p <= 256, so the remainder is
// composed from 32-bit halves: h = hi * 2^32 + lo and every intermediate
// stays below 2^16.  That avoids the emulated 64-bit division.
DEV_INLINE int part_id(uint64_t h, const PartSpec s) {
  if (s.remix) h = splitmix64(h);
  if (s.pow2) return (int)(h & (uint64_t)(s.p - 1));
  uint32_t hi = (uint32_t)(h >> 32), lo = (uint32_t)h;
  return (int)(((hi % s.p) * s.two32 + lo % s.p) % s.p);
}

// Lanes of this wave that are active and hold the same id as the caller.
// Every lane of the wave must call it (ballots are wave-wide).
DEV_INLINE uint64_t part_peers(int d, bool active, int bits) {
  uint64_t peers = __ballot(active);
  for (int b = 0; b < bits; ++b) {
    bool bit = (d >> b) & 1;
    uint64_t vote = __ballot(bit);
    peers &= bit ? vote : ~vote;
  }
  return peers;
}

// hist[b][d] = rows of block b's chunk that fall in partition d.  A wave
// adds one count per distinct id, so a skewed input does not serialise on
// one LDS counter.
__global__ void partition_hist_kernel(const uint64_t* hashes, int64_t n,
                                      int64_t chunk, PartSpec spec,
                                      int64_t* hist /*[nblocks][p]*/) {
  __shared__ int32_t lhist[PART_MAX];
  const int P = (int)spec.p;
  for (int d = threadIdx.x; d < P; d += blockDim.x) lhist[d] = 0;
  __syncthreads();
  int64_t begin = (int64_t)blockIdx.x * chunk;
  int64_t end = min(begin + chunk, n);
  int lane = threadIdx.x & (WAVE - 1);
  uint64_t lane_lt = (1ull << lane) - 1;
  for (int64_t tile = begin; tile < end; tile += PART_BLOCK) {
    int64_t i = tile + threadIdx.x;
    bool active = i < end;
    int d = active ? part_id(hashes[i], spec) : 0;
    uint64_t peers = part_peers(d, active, spec.bits);
    if (active && (peers & lane_lt) == 0)
      atomicAdd(&lhist[d], __popcll(peers));
  }
  __syncthreads();
  for (int d = threadIdx.x; d < P; d += blockDim.x)
    hist[(int64_t)blockIdx.x * P + d] = (int64_t)lhist[d];
}

// Stable scatter: block b owns rows [b*chunk, (b+1)*chunk), walked as
// 256-row tiles.  running[d] is the next free slot of partition d for this
// block; within a tile a row's slot is running[d] + rows of earlier waves
// with id d + its rank among its wave's peers.
__global__ void partition_scatter_kernel(const uint64_t* hashes, int64_t n,
                                         int64_t chunk, PartSpec spec,
                                         const int64_t* offsets /*[nb][p]*/,
                                         int64_t* perm) {
  __shared__ int64_t running[PART_MAX];
  __shared__ int32_t wave_hist[PART_NWAVES][PART_MAX];
  const int P = (int)spec.p;
  for (int d = threadIdx.x; d < P; d += blockDim.x)
    running[d] = offsets[(int64_t)blockIdx.x * P + d];
  int64_t begin = (int64_t)blockIdx.x * chunk;
  int64_t end = min(begin + chunk, n);
  int lane = threadIdx.x & (WAVE - 1);
  int wid = threadIdx.x / WAVE;
  uint64_t lane_lt = (1ull << lane) - 1;
  for (int64_t tile = begin; tile < end; tile += PART_BLOCK) {
    for (int d = threadIdx.x; d < P; d += blockDim.x)
      for (int w = 0; w < PART_NWAVES; ++w) wave_hist[w][d] = 0;
    __syncthreads();
    int64_t i = tile + threadIdx.x;
    bool active = i < end;
    int d = active ? part_id(hashes[i], spec) : 0;
    uint64_t peers = part_peers(d, active, spec.bits);
    int rank_in_wave = __popcll(peers & lane_lt);
    if (active && rank_in_wave == 0) wave_hist[wid][d] = __popcll(peers);
    __syncthreads();
    if (active) {
      int32_t before = 0;
      for (int w = 0; w < wid; ++w) before += wave_hist[w][d];
      perm[running[d] + before + rank_in_wave] = i;
    }
    __syncthreads();
    for (int d2 = threadIdx.x; d2 < P; d2 += blockDim.x) {
      int32_t t = 0;
      for (int w = 0; w < PART_NWAVES; ++w) t += wave_hist[w][d2];
      running[d2] += t;
    }
    __syncthreads();
  }
}

std::vector<Tensor> hash_partition(Tensor hashes, int64_t num_partitions,
                                   bool remix) {
  TORCH_CHECK(hashes.is_cuda() && hashes.dtype() == torch::kInt64 &&
                  hashes.dim() == 1,
              "hash_partition: hashes must be a 1-D int64 device tensor");
  TORCH_CHECK(num_partitions >= 1 && num_partitions <= PART_MAX,
              "hash_partition: num_partitions must be in [1, ", PART_MAX,
              "], got ", num_partitions);
  hashes = hashes.contiguous();
  auto dev = hashes.device();
  int64_t n = hashes.numel();
  auto opts64 = torch::dtype(torch::kInt64).device(dev);
  if (n == 0)
    return {torch::empty({0}, opts64), torch::zeros({num_partitions}, opts64)};

  PartSpec spec;
  spec.p = (uint32_t)num_partitions;
  spec.two32 = (uint32_t)((1ull << 32) % (uint64_t)num_partitions);
  spec.bits = 0;
  while ((1 << spec.bits) < num_partitions) ++spec.bits;
  spec.pow2 = (num_partitions & (num_partitions - 1)) == 0;
  spec.remix = remix;

  int64_t chunk = (n + kMaxBlocks - 1) / kMaxBlocks;
  if (chunk < PART_BLOCK) chunk = PART_BLOCK;
  // a block counts its chunk in int32 LDS cells
  TORCH_CHECK(chunk <= INT32_MAX, "hash_partition: too many rows");
  int nblocks = (int)((n + chunk - 1) / chunk);
  auto stream = cur_stream();
  const uint64_t* hp = (const uint64_t*)hashes.data_ptr<int64_t>();

  auto hist = torch::empty({(int64_t)nblocks, num_partitions}, opts64);
  hipLaunchKernelGGL(partition_hist_kernel, dim3(nblocks), dim3(PART_BLOCK),
                     0, stream, hp, n, chunk, spec, hist.data_ptr<int64_t>());
  auto counts = hist.sum(0);
  auto part_base = torch::cumsum(counts, 0) - counts;   // exclusive
  auto block_excl = torch::cumsum(hist, 0) - hist;
  auto offsets = (part_base.unsqueeze(0) + block_excl).contiguous();
  auto perm = torch::empty({n}, opts64);
  hipLaunchKernelGGL(partition_scatter_kernel, dim3(nblocks),
                     dim3(PART_BLOCK), 0, stream, hp, n, chunk, spec,
                     offsets.data_ptr<int64_t>(), perm.data_ptr<int64_t>());
  return {perm, counts};
}
