// Top-k candidate selection on order-encoded u64 keys (gfx950): an MSD radix
// select that finds T, the k-th smallest key, and returns every row whose key
// is <= T in ascending row order.  TopN (rowops.topk_multi) sorts only those
// rows; a full radix_argsort of the input moves a 16 B key/row pair eight
// times to keep a handful of rows.
//
// All selection state lives in one device struct (TopkState); the host reads
// it once, at the end, to size the output.
//   span   one pass, 16 B loads: AND and OR of all keys.  vary = and ^ or.
//          Order keys of real columns (sign-flipped small ints, dates,
//          dictionary ranks) share long prefixes, so digits are placed only
//          over bits that vary: a 20-bit value range costs two histogram
//          passes, an all-equal column none.
//   hist   one launch per pass.  Rows with (key & decided) == prefix count
//          their 11-bit digit at `shift` into a 2048-bin LDS histogram;
//          non-zero bins are added to a global int64 [2048].
//   pick   one block: scans the bins, finds the one where the running count
//          crosses k_rem, folds it into prefix/decided, moves the rows below
//          it into n_less, places the next digit with its top at the highest
//          undecided varying bit (or sets done), and zeroes the histogram.
//   The launcher enqueues ceil(64 / 11) = 6 hist/pick pairs unconditionally;
//   the ones after `done` return on their first load.
//   count / write   a fused stable compaction of keys <= T: per-block counts,
//          a device cumsum, then ballot-ranked writes of the row numbers.
//
// Skew in the LDS histogram: after the first pass the surviving rows of a
// wave usually share one digit (a long run of equal keys, a heavy bin).  The
// wave takes the digit of its first participating lane, and all lanes that
// hold it are added with one atomicAdd of the ballot popcount; the remaining
// lanes add 1 each.  That is two ballots per key slot.  wave_peers
// (block_rank.h) ranks every distinct digit, which would take 11 ballot
// rounds here and buys nothing for spread-out digits, where LDS atomics do
// not collide anyway.
//
// Block decomposition, block counts and compaction slots are the steps of
// block_rank.h; all row arithmetic is int64, so the row count is not capped
// at 2^31.  chunk is even, so every block starts on a 16-byte boundary and a
// thread loads two keys at a time.
#include "common.h"
#include "block_rank.h"
#include "host_args.h"
#include "api.h"

constexpr int TOPK_BITS = 11;
constexpr int TOPK_BINS = 1 << TOPK_BITS;          // 2048 int32 = 8 KB LDS
constexpr int TOPK_PASSES = (64 + TOPK_BITS - 1) / TOPK_BITS;
constexpr int TOPK_BLOCK = 256;
constexpr int TOPK_NWAVES = TOPK_BLOCK / WAVE;
constexpr int TOPK_TILE = 2 * TOPK_BLOCK;          // keys per block step
constexpr int TOPK_PER_THREAD = TOPK_BINS / TOPK_BLOCK;  // bins in pick

// int64 [TOPK_STATE_WORDS] on the device; the first three words are `stats`
struct TopkState {
  uint64_t threshold;     // T, valid once done
  int64_t n_less;         // keys < prefix on the decided bits
  int64_t n_match;        // keys equal to prefix on the decided bits
  uint64_t prefix;        // decided bits of T
  uint64_t decided_mask;
  uint64_t vary_mask;
  uint64_t and_bits;      // AND of all keys (bits of T that never vary)
  uint64_t or_bits;
  int64_t k_rem;          // 1-based rank of T among the matching rows
  int32_t shift;          // low bit of the current digit
  int32_t done;
};
constexpr int TOPK_STATE_WORDS = sizeof(TopkState) / sizeof(int64_t);
static_assert(sizeof(TopkState) % sizeof(int64_t) == 0, "state is int64 words");

// two keys per thread: rows i and i + 1 of [.., end), i even
struct KeyPair {
  uint64_t k0, k1;
  bool a0, a1;
};

DEV_INLINE KeyPair load_pair(const uint64_t* keys, int64_t i, int64_t end) {
  KeyPair p{0, 0, i < end, i + 1 < end};
  if (p.a1) {
    ulonglong2 v = *reinterpret_cast<const ulonglong2*>(keys + i);
    p.k0 = v.x;
    p.k1 = v.y;
  } else if (p.a0) {
    p.k0 = keys[i];
  }
  return p;
}

// Place the next digit, or finish: nothing undecided varies any more, so
// every matching row equals T.
DEV_INLINE void topk_advance(TopkState* s) {
  uint64_t open = s->vary_mask & ~s->decided_mask;
  if (open == 0) {
    s->threshold = s->prefix | (s->and_bits & ~s->decided_mask);
    s->done = 1;
    return;
  }
  int top = 63 - __clzll((long long)open);
  s->shift = max(top - (TOPK_BITS - 1), 0);
}

__global__ void topk_init_kernel(TopkState* s, int64_t* hist, int64_t n,
                                 int64_t k) {
  for (int d = threadIdx.x; d < TOPK_BINS; d += blockDim.x) hist[d] = 0;
  if (threadIdx.x == 0) {
    s->threshold = 0;
    s->n_less = 0;
    s->n_match = n;
    s->prefix = 0;
    s->decided_mask = 0;
    s->vary_mask = 0;
    s->and_bits = ~0ull;
    s->or_bits = 0;
    s->k_rem = k;
    s->shift = 0;
    s->done = 0;
  }
}

__global__ void topk_span_kernel(const uint64_t* keys, int64_t n,
                                 TopkState* s) {
  __shared__ uint64_t wand[TOPK_NWAVES], wor[TOPK_NWAVES];
  uint64_t a = ~0ull, o = 0;
  int64_t stride = (int64_t)gridDim.x * TOPK_TILE;
  for (int64_t i = (int64_t)blockIdx.x * TOPK_TILE + 2 * threadIdx.x; i < n;
       i += stride) {
    KeyPair p = load_pair(keys, i, n);
    a &= p.k0;
    o |= p.k0;
    if (p.a1) {
      a &= p.k1;
      o |= p.k1;
    }
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    a &= (uint64_t)__shfl_xor((unsigned long long)a, off);
    o |= (uint64_t)__shfl_xor((unsigned long long)o, off);
  }
  if (lane_id() == 0) {
    wand[wave_id()] = a;
    wor[wave_id()] = o;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < TOPK_NWAVES; ++w) {
      a &= wand[w];
      o |= wor[w];
    }
    atomicAnd((unsigned long long*)&s->and_bits, (unsigned long long)a);
    atomicOr((unsigned long long*)&s->or_bits, (unsigned long long)o);
  }
}

__global__ void topk_plan_kernel(TopkState* s) {
  s->vary_mask = s->and_bits ^ s->or_bits;
  topk_advance(s);
}

// One key slot of a wave into the LDS histogram.  Every lane of the wave
// must call it (ballots are wave-wide).
DEV_INLINE void topk_count_digit(int32_t* lhist, int d, bool part, int lane) {
  uint64_t act = __ballot(part);
  if (act == 0) return;
  int lead = __ffsll((long long)act) - 1;
  int d0 = __shfl(d, lead);
  uint64_t same = __ballot(part && d == d0);
  if (!part) return;
  if (d != d0)
    atomicAdd(&lhist[d], 1);
  else if (lane == lead)
    atomicAdd(&lhist[d0], __popcll(same));
}

__global__ void topk_hist_kernel(const uint64_t* keys, int64_t n,
                                 int64_t chunk, const TopkState* s,
                                 int64_t* hist /*[TOPK_BINS]*/) {
  __shared__ int32_t lhist[TOPK_BINS];
  if (s->done) return;
  const uint64_t prefix = s->prefix, decided = s->decided_mask;
  const int shift = s->shift;
  for (int d = threadIdx.x; d < TOPK_BINS; d += blockDim.x) lhist[d] = 0;
  __syncthreads();
  int64_t begin = (int64_t)blockIdx.x * chunk;
  int64_t end = min(begin + chunk, n);
  int lane = lane_id();
  for (int64_t tile = begin; tile < end; tile += TOPK_TILE) {
    KeyPair p = load_pair(keys, tile + 2 * threadIdx.x, end);
    topk_count_digit(lhist, (int)((p.k0 >> shift) & (TOPK_BINS - 1)),
                     p.a0 && (p.k0 & decided) == prefix, lane);
    topk_count_digit(lhist, (int)((p.k1 >> shift) & (TOPK_BINS - 1)),
                     p.a1 && (p.k1 & decided) == prefix, lane);
  }
  __syncthreads();
  for (int d = threadIdx.x; d < TOPK_BINS; d += blockDim.x)
    if (lhist[d])
      atomicAdd((unsigned long long*)&hist[d], (unsigned long long)lhist[d]);
}

// One block.  Thread t owns bins [8t, 8t + 8); an inclusive scan of the
// per-thread sums finds the thread, then the bin, where the count crosses
// k_rem.
__global__ void topk_pick_kernel(TopkState* s, int64_t* hist) {
  __shared__ int64_t scan[2][TOPK_BLOCK];
  if (s->done) return;
  const int64_t k_rem = s->k_rem;
  const int shift = s->shift;
  const int t = threadIdx.x;
  int64_t c[TOPK_PER_THREAD], sum = 0;
  for (int j = 0; j < TOPK_PER_THREAD; ++j) {
    c[j] = hist[t * TOPK_PER_THREAD + j];
    hist[t * TOPK_PER_THREAD + j] = 0;
    sum += c[j];
  }
  int cur = 0;
  scan[0][t] = sum;
  __syncthreads();
  for (int off = 1; off < TOPK_BLOCK; off <<= 1) {
    int64_t v = scan[cur][t] + (t >= off ? scan[cur][t - off] : 0);
    scan[cur ^ 1][t] = v;
    cur ^= 1;
    __syncthreads();
  }
  int64_t below = scan[cur][t] - sum;
  if (below < k_rem && k_rem <= below + sum) {
    int j = 0;
    while (below + c[j] < k_rem) below += c[j++];
    uint64_t mask = (uint64_t)(TOPK_BINS - 1) << shift;
    uint64_t bin = (uint64_t)(t * TOPK_PER_THREAD + j);
    s->prefix = (s->prefix & ~mask) | (bin << shift);
    s->decided_mask |= mask;
    s->n_less += below;
    s->k_rem = k_rem - below;
    s->n_match = c[j];
    topk_advance(s);
  }
}

// cnt[b] = rows of block b's chunk with key <= T
__global__ void topk_count_kernel(const uint64_t* keys, int64_t n,
                                  int64_t chunk, const TopkState* s,
                                  int64_t* cnt /*[nblocks]*/) {
  const uint64_t T = s->threshold;
  int64_t begin = (int64_t)blockIdx.x * chunk;
  int64_t end = min(begin + chunk, n);
  int32_t mine = 0;
  for (int64_t tile = begin; tile < end; tile += TOPK_TILE) {
    KeyPair p = load_pair(keys, tile + 2 * threadIdx.x, end);
    mine += (int)(p.a0 && p.k0 <= T) + (int)(p.a1 && p.k1 <= T);
  }
  int32_t total = block_sum(mine);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// Stable write: rows[base[b] ..] = the block's rows with key <= T, in row
// order (two ballots, one per key slot).  wtot is double-buffered by tile
// parity, so one barrier per tile is enough.
__global__ void topk_write_kernel(const uint64_t* keys, int64_t n,
                                  int64_t chunk, const TopkState* s,
                                  const int64_t* base /*[nblocks]*/,
                                  int64_t* rows, int64_t m) {
  __shared__ int32_t wtot[2][TOPK_NWAVES];
  const uint64_t T = s->threshold;
  int64_t begin = (int64_t)blockIdx.x * chunk;
  int64_t end = min(begin + chunk, n);
  int64_t run = base[blockIdx.x];
  int buf = 0;
  for (int64_t tile = begin; tile < end; tile += TOPK_TILE, buf ^= 1) {
    int64_t i = tile + 2 * threadIdx.x;
    KeyPair p = load_pair(keys, i, end);
    bool f0 = p.a0 && p.k0 <= T, f1 = p.a1 && p.k1 <= T;
    int t0, t1;
    int r0 = wave_rank(f0, &t0), r1 = wave_rank(f1, &t1);
    wave_total_put(wtot[buf], t0 + t1);
    __syncthreads();
    WaveSpan w = wave_span<TOPK_NWAVES>(wtot[buf]);
    int64_t pos = run + w.before + r0 + r1;
    // pos < m whenever the counts agree with the state; the check keeps a
    // disagreement from writing past the buffer
    if (f0 && pos < m) rows[pos] = i;
    if (f1 && pos + f0 < m) rows[pos + f0] = i + 1;
    run += w.total;
  }
}

std::vector<Tensor> topk_candidates(Tensor keys, int64_t k) {
  const char* who = "topk_candidates";
  TORCH_CHECK(keys.is_cuda() && keys.dim() == 1, who,
              ": keys must be a 1-D device tensor");
  check_tensor(who, "keys", keys, torch::kInt64, keys.device());
  int64_t n = keys.numel();
  TORCH_CHECK(k >= 1 && k <= n, who, ": k must be in [1, ", n, "], got ", k);
  // a slice can start 8 bytes off the 16-byte boundary the loads need
  if (reinterpret_cast<uintptr_t>(keys.data_ptr<int64_t>()) % 16 != 0)
    keys = keys.clone();
  auto opts64 = torch::dtype(torch::kInt64).device(keys.device());

  auto [chunk, nblocks] = block_chunks(n, TOPK_TILE, 2);
  // a block counts its chunk in int32 LDS cells
  TORCH_CHECK(chunk <= INT32_MAX - 1, who, ": too many rows");
  auto stream = cur_stream();
  const uint64_t* kp = (const uint64_t*)keys.data_ptr<int64_t>();

  auto state = torch::empty({TOPK_STATE_WORDS}, opts64);
  auto hist = torch::empty({TOPK_BINS}, opts64);
  auto* sp = reinterpret_cast<TopkState*>(state.data_ptr<int64_t>());
  int64_t* hp = hist.data_ptr<int64_t>();
  hipLaunchKernelGGL(topk_init_kernel, dim3(1), dim3(TOPK_BLOCK), 0, stream,
                     sp, hp, n, k);
  hipLaunchKernelGGL(topk_span_kernel, dim3(grid_1d(n, TOPK_BLOCK, 2)),
                     dim3(TOPK_BLOCK), 0, stream, kp, n, sp);
  hipLaunchKernelGGL(topk_plan_kernel, dim3(1), dim3(1), 0, stream, sp);
  for (int pass = 0; pass < TOPK_PASSES; ++pass) {
    hipLaunchKernelGGL(topk_hist_kernel, dim3(nblocks), dim3(TOPK_BLOCK), 0,
                       stream, kp, n, chunk, sp, hp);
    hipLaunchKernelGGL(topk_pick_kernel, dim3(1), dim3(TOPK_BLOCK), 0, stream,
                       sp, hp);
  }
  auto cnt = torch::empty({(int64_t)nblocks}, opts64);
  hipLaunchKernelGGL(topk_count_kernel, dim3(nblocks), dim3(TOPK_BLOCK), 0,
                     stream, kp, n, chunk, sp, cnt.data_ptr<int64_t>());
  auto base = (torch::cumsum(cnt, 0) - cnt).contiguous();

  auto stats = state.slice(0, 0, 3);
  auto host = state.cpu();                       // the one sync
  auto* hs = reinterpret_cast<const TopkState*>(host.data_ptr<int64_t>());
  int64_t m = hs->n_less + hs->n_match;
  TORCH_CHECK(hs->done && m >= k && m <= n, who,
              ": selection did not converge (done=", hs->done, ", m=", m, ")");
  auto rows = torch::empty({m}, opts64);
  hipLaunchKernelGGL(topk_write_kernel, dim3(nblocks), dim3(TOPK_BLOCK), 0,
                     stream, kp, n, chunk, sp, base.data_ptr<int64_t>(),
                     rows.data_ptr<int64_t>(), m);
  return {rows, stats};
}
