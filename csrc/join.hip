// Join kernels for gfx950.
//  * direct-address join: the build side is one unique integer key over a
//    small range, so the "hash table" is an int32 row array indexed by
//    key - min.  The probe is one coalesced key load plus one table lookup
//    per row; the table stays in L2 / Infinity Cache for the PK-join shapes.
//  * bucket-chain hash join: build + verified probe.  The probe walks each
//    chain once: pass one records the first matching build row next to the
//    count, pass two writes rows with at most one output straight from that
//    record and resumes the walk there for rows with fan-out.
// Both probes emit (lidx, ridx) int64 gather maps with lidx ascending.

#include <limits>

#include "common.h"
#include "host_args.h"
#include "row_ops.h"
#include "api.h"

enum JoinMode : int { JOIN_INNER = 0, JOIN_LEFT = 1, JOIN_SEMI = 2,
                      JOIN_ANTI = 3 };

constexpr int kJoinBlock = 256;
constexpr int kJoinWaves = kJoinBlock / WAVE;
// tiles a block has in flight per loop trip: the lookups of one trip are
// independent, so their latencies overlap
constexpr int kJoinUnroll = 4;

// ---------------------------------------------------------------------------
// direct-address join
// ---------------------------------------------------------------------------

// table[key - mn] = build row.  With CHECK_DUP a slot is claimed by
// compare-and-swap from -1 and a second claimant raises *dup; without it
// (semi/anti: existence only) any winner may stay.
template <typename K, bool CHECK_DUP>
__global__ void dense_build_kernel(const K* keys, int64_t n, int64_t mn,
                                   int64_t rng, int32_t* table,
                                   int32_t* dup) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t k = (int64_t)keys[i];
    if (k < mn || k - mn >= rng) continue;  // cannot happen: mn/rng are theirs
    if constexpr (CHECK_DUP) {
      if (atomicCAS(&table[k - mn], -1, (int32_t)i) != -1) atomicOr(dup, 1);
    } else {
      table[k - mn] = (int32_t)i;
    }
  }
}

// Build row of probe row i, or -1.  Out-of-range and null keys never match.
// Branch-free on purpose (a miss reads slot 0) so that the lookups of an
// unrolled loop issue back to back.
template <typename K>
DEV_INLINE int32_t dense_lookup(const K* keys, const bool* valid, int64_t i,
                                int64_t mn, int64_t mx,
                                const int32_t* table) {
  int64_t k = (int64_t)keys[i];
  bool in = k >= mn && k <= mx;
  if (valid) in = in && valid[i];
  int32_t row = table[in ? k - mn : 0];
  return in ? row : -1;
}

// Count pass: block b counts the selected rows of [b*chunk, (b+1)*chunk).
// A row is selected when it has a build row, or for ANTI when it has none.
// The looked-up rows are kept (4 B per probe row) so that the fill pass
// streams them back and the table is read once per probe row: with random
// keys over a table beyond L2 the lookup is what the pass costs.
template <typename K>
__global__ void dense_count_kernel(const K* keys, const bool* valid,
                                   int64_t n, int64_t chunk, int64_t mn,
                                   int64_t mx, const int32_t* table,
                                   bool anti, int32_t* rows,
                                   int64_t* counts) {
  int64_t begin = (int64_t)blockIdx.x * chunk;
  int64_t end = min(begin + chunk, n);
  int32_t local = 0;
#pragma unroll kJoinUnroll
  for (int64_t i = begin + threadIdx.x; i < end; i += kJoinBlock) {
    int32_t row = dense_lookup(keys, valid, i, mn, mx, table);
    rows[i] = row;
    local += ((row >= 0) != anti);
  }
  __shared__ int32_t acc;
  if (threadIdx.x == 0) acc = 0;
  __syncthreads();
  for (int off = WAVE / 2; off; off >>= 1)
    local += __shfl_down(local, off, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) atomicAdd(&acc, local);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = acc;
}

// Fill pass: same chunks, kJoinUnroll tiles per trip, ballot rank within the
// wave and wave totals through LDS, so output order is row order.
// rows is what the count pass looked up; incl is the inclusive scan of
// counts; ridx is null for semi/anti.
__global__ void dense_fill_kernel(const int32_t* rows, int64_t n,
                                  int64_t chunk, bool anti,
                                  const int64_t* incl, const int64_t* counts,
                                  int64_t* lidx, int64_t* ridx) {
  int64_t begin = (int64_t)blockIdx.x * chunk;
  int64_t end = min(begin + chunk, n);
  __shared__ int32_t wave_counts[kJoinUnroll][kJoinWaves];
  int64_t base = incl[blockIdx.x] - counts[blockIdx.x];
  int lane = threadIdx.x & (WAVE - 1);
  int wid = threadIdx.x / WAVE;
  for (int64_t tile = begin; tile < end;
       tile += (int64_t)kJoinUnroll * kJoinBlock) {
    int32_t row[kJoinUnroll];
#pragma unroll
    for (int u = 0; u < kJoinUnroll; ++u) {
      int64_t i = tile + u * kJoinBlock + threadIdx.x;
      row[u] = i < end ? rows[i] : -2;
    }
    int rank[kJoinUnroll];
    bool sel[kJoinUnroll];
#pragma unroll
    for (int u = 0; u < kJoinUnroll; ++u) {
      // -2 marks a row past the end: selected by no mode
      sel[u] = anti ? row[u] == -1 : row[u] >= 0;
      uint64_t ballot = __ballot(sel[u]);
      rank[u] = __popcll(ballot & ((1ull << lane) - 1));
      if (lane == 0) wave_counts[u][wid] = __popcll(ballot);
    }
    __syncthreads();
    int64_t pos = base;
#pragma unroll
    for (int u = 0; u < kJoinUnroll; ++u) {
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kJoinWaves; ++w) {
        int c = wave_counts[u][w];
        before += w < wid ? c : 0;
        total += c;
      }
      if (sel[u]) {
        int64_t o = pos + before + rank[u];
        lidx[o] = tile + u * kJoinBlock + threadIdx.x;
        if (ridx) ridx[o] = row[u];
      }
      pos += total;
    }
    base = pos;  // every thread keeps the same running base
    __syncthreads();
  }
}

// Left join: no compaction, one pass.
template <typename K>
__global__ void dense_left_kernel(const K* keys, const bool* valid, int64_t n,
                                  int64_t mn, int64_t mx,
                                  const int32_t* table, int64_t* lidx,
                                  int64_t* ridx) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
#pragma unroll kJoinUnroll
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    lidx[i] = i;
    ridx[i] = dense_lookup(keys, valid, i, mn, mx, table);
  }
}

static void check_dense_keys(const Tensor& keys) {
  TORCH_CHECK(keys.is_cuda() && keys.dim() == 1 && keys.is_contiguous() &&
                  (keys.dtype() == torch::kInt32 ||
                   keys.dtype() == torch::kInt64),
              "dense join keys must be contiguous int32/int64 on the GPU");
}

template <typename K>
static void launch_dense_build(const Tensor& keys, int64_t mn, int64_t rng,
                               bool check_dup, Tensor& table, Tensor& dup) {
  int64_t n = keys.numel();
  auto kern = check_dup ? dense_build_kernel<K, true>
                        : dense_build_kernel<K, false>;
  hipLaunchKernelGGL(kern, dim3(grid_1d(n, kJoinBlock)), dim3(kJoinBlock), 0,
                     cur_stream(), keys.data_ptr<K>(), n, mn, rng,
                     table.data_ptr<int32_t>(), dup.data_ptr<int32_t>());
}

std::vector<Tensor> dense_join_build(Tensor keys, int64_t mn, int64_t rng,
                                     bool check_dup) {
  check_dense_keys(keys);
  int64_t n = keys.numel();
  TORCH_CHECK(n < (int64_t)1 << 31, "dense_join_build: n_r must fit int32");
  TORCH_CHECK(rng >= 1, "dense_join_build: empty key range");
  auto opts32 = torch::dtype(torch::kInt32).device(keys.device());
  auto table = torch::full({rng}, -1, opts32);
  auto dup = torch::zeros({1}, opts32);
  if (n > 0) {
    if (keys.dtype() == torch::kInt32)
      launch_dense_build<int32_t>(keys, mn, rng, check_dup, table, dup);
    else
      launch_dense_build<int64_t>(keys, mn, rng, check_dup, table, dup);
  }
  return {table, dup};
}

template <typename K>
static std::vector<Tensor> dense_probe_t(const Tensor& keys,
                                         const bool* valid, int64_t mn,
                                         const Tensor& table, int mode) {
  auto dev = keys.device();
  auto opts64 = torch::dtype(torch::kInt64).device(dev);
  int64_t n = keys.numel();
  int64_t mx = mn + table.numel() - 1;
  const K* kp = keys.data_ptr<K>();
  const int32_t* tp = table.data_ptr<int32_t>();
  if (mode == JOIN_LEFT) {
    auto lidx = torch::empty({n}, opts64);
    auto ridx = torch::empty({n}, opts64);
    hipLaunchKernelGGL(dense_left_kernel<K>, dim3(grid_1d(n, kJoinBlock)),
                       dim3(kJoinBlock), 0, cur_stream(), kp, valid, n, mn,
                       mx, tp, lidx.data_ptr<int64_t>(),
                       ridx.data_ptr<int64_t>());
    return {lidx, ridx};
  }
  bool anti = mode == JOIN_ANTI;
  int64_t tile = (int64_t)kJoinUnroll * kJoinBlock;
  int64_t chunk = (n + kMaxBlocks - 1) / kMaxBlocks;
  chunk = (chunk + tile - 1) / tile * tile;
  int nblocks = (int)((n + chunk - 1) / chunk);
  auto counts = torch::empty({nblocks}, opts64);
  auto rows = torch::empty({n}, torch::dtype(torch::kInt32).device(dev));
  hipLaunchKernelGGL(dense_count_kernel<K>, dim3(nblocks), dim3(kJoinBlock),
                     0, cur_stream(), kp, valid, n, chunk, mn, mx, tp, anti,
                     rows.data_ptr<int32_t>(), counts.data_ptr<int64_t>());
  auto incl = torch::cumsum(counts, 0);
  int64_t total = incl[nblocks - 1].item<int64_t>();
  auto lidx = torch::empty({total}, opts64);
  auto ridx = torch::empty({mode == JOIN_INNER ? total : 0}, opts64);
  if (total > 0)
    hipLaunchKernelGGL(dense_fill_kernel, dim3(nblocks), dim3(kJoinBlock), 0,
                       cur_stream(), rows.data_ptr<int32_t>(), n, chunk, anti,
                       incl.data_ptr<int64_t>(), counts.data_ptr<int64_t>(),
                       lidx.data_ptr<int64_t>(),
                       mode == JOIN_INNER ? ridx.data_ptr<int64_t>()
                                          : nullptr);
  return {lidx, ridx};
}

std::vector<Tensor> dense_join_probe(Tensor keys, OptTensor valid, int64_t mn,
                                     Tensor table, int64_t mode) {
  check_dense_keys(keys);
  TORCH_CHECK(table.is_cuda() && table.dtype() == torch::kInt32 &&
              table.is_contiguous() && table.numel() >= 1);
  TORCH_CHECK(mode >= JOIN_INNER && mode <= JOIN_ANTI);
  TORCH_CHECK(mn <= std::numeric_limits<int64_t>::max() - table.numel());
  int64_t n = keys.numel();
  auto opts64 = torch::dtype(torch::kInt64).device(keys.device());
  if (n == 0) return {torch::empty({0}, opts64), torch::empty({0}, opts64)};
  const bool* vp = nullptr;
  Tensor v;
  if (valid.has_value()) {
    v = valid->contiguous();
    TORCH_CHECK(v.is_cuda() && v.dtype() == torch::kBool && v.numel() == n);
    vp = v.data_ptr<bool>();
  }
  if (keys.dtype() == torch::kInt32)
    return dense_probe_t<int32_t>(keys, vp, mn, table, (int)mode);
  return dense_probe_t<int64_t>(keys, vp, mn, table, (int)mode);
}

// ---------------------------------------------------------------------------
// hash join: bucket-chain build + verified probe
// ---------------------------------------------------------------------------

__global__ void join_build_kernel(const uint64_t* hashes, int64_t n,
                                  int64_t* heads, int64_t* next,
                                  uint64_t mask) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    uint64_t b = hashes[i] & mask;
    long long prev = atomicExch((unsigned long long*)&heads[b],
                                (unsigned long long)i);
    next[i] = prev;
  }
}

std::vector<Tensor> join_build(Tensor hashes) {
  auto dev = hashes.device();
  int64_t n = hashes.numel();
  auto opts64 = torch::dtype(torch::kInt64).device(dev);
  int64_t cap = table_capacity(std::max<int64_t>(n, 1));
  auto heads = torch::full({cap}, -1, opts64);
  auto next = torch::full({std::max<int64_t>(n, 1)}, -1, opts64);
  if (n > 0) {
    hipLaunchKernelGGL(join_build_kernel, dim3(grid_1d(n, kJoinBlock)),
                       dim3(kJoinBlock), 0, cur_stream(),
                       (const uint64_t*)hashes.data_ptr<int64_t>(), n,
                       heads.data_ptr<int64_t>(), next.data_ptr<int64_t>(),
                       (uint64_t)(cap - 1));
  }
  return {heads, next};
}

struct ProbeArgs {
  const int64_t* heads;
  const int64_t* next;
  const uint64_t* ph;
  const uint64_t* bh;
  const ColDesc* pc;
  const ColDesc* bc;
  int ncols;
  int64_t np;
  uint64_t mask;
};

DEV_INLINE bool probe_match(const ProbeArgs& a, uint64_t h, int64_t i,
                            int64_t j) {
  return a.bh[j] == h && row_eq(a.pc, a.bc, a.ncols, i, j, false);
}

// Pass one, the only full chain walk.  EXISTS (semi/anti) stops at the first
// match and writes flag[i] = row selected; otherwise first[i] is the first
// matching build row in chain order (-1: none) and counts[i] the number of
// output rows (LEFT emits one for a row without a match).  F is int32 when
// the build side has fewer than 2^31 rows.
template <typename F, bool EXISTS>
__global__ void join_probe_count_kernel(ProbeArgs a, int mode, F* first,
                                        int32_t* counts, bool* flag) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.np;
       i += stride) {
    uint64_t h = a.ph[i];
    int64_t m = 0, f = -1;
    if (!row_has_null(a.pc, a.ncols, i)) {
      int64_t j = a.heads[h & a.mask];
      while (j != -1) {
        if (probe_match(a, h, i, j)) {
          if (m++ == 0) f = j;
          if constexpr (EXISTS) break;
        }
        j = a.next[j];
      }
    }
    if constexpr (EXISTS) {
      flag[i] = (m != 0) == (mode == JOIN_SEMI);
    } else {
      first[i] = (F)f;
      counts[i] = (int32_t)(mode == JOIN_LEFT && m == 0 ? 1 : m);
    }
  }
}

// Pass two (inner/left).  Row i owns outputs [incl[i]-counts[i], incl[i]).
// One output: written from first[i] alone.  More: the walk resumes at
// first[i], which is known to match, and stops once all are out.
template <typename F>
__global__ void join_probe_fill_kernel(ProbeArgs a, const F* first,
                                       const int32_t* counts,
                                       const int64_t* incl, int64_t* lidx,
                                       int64_t* ridx, bool* matched) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.np;
       i += stride) {
    int32_t c = counts[i];
    if (c == 0) continue;
    int64_t pos = incl[i] - c;
    int64_t j = (int64_t)first[i];
    lidx[pos] = i;
    ridx[pos] = j;  // -1: the null row of a left join
    if (j < 0) continue;
    if (matched) matched[j] = true;
    if (c == 1) continue;
    uint64_t h = a.ph[i];
    int64_t end = pos + c;
    ++pos;
    for (j = a.next[j]; pos < end && j != -1; j = a.next[j]) {
      if (probe_match(a, h, i, j)) {
        lidx[pos] = i;
        ridx[pos] = j;
        if (matched) matched[j] = true;
        ++pos;
      }
    }
  }
}

template <typename F>
static std::vector<Tensor> join_probe_t(const ProbeArgs& a, int mode,
                                        int64_t nb, bool need_matched,
                                        c10::Device dev) {
  auto opts64 = torch::dtype(torch::kInt64).device(dev);
  auto optsb = torch::dtype(torch::kBool).device(dev);
  int64_t np = a.np;
  dim3 grid(grid_1d(np, kJoinBlock)), block(kJoinBlock);
  Tensor matched = need_matched ? torch::zeros({nb}, optsb)
                                : torch::empty({0}, optsb);
  if (np == 0)
    return {torch::empty({0}, opts64), torch::empty({0}, opts64), matched};
  if (mode >= JOIN_SEMI) {
    auto flag = torch::empty({np}, optsb);
    hipLaunchKernelGGL((join_probe_count_kernel<F, true>), grid, block, 0,
                       cur_stream(), a, mode, (F*)nullptr, (int32_t*)nullptr,
                       flag.data_ptr<bool>());
    return {compact_indices(flag), torch::empty({0}, opts64), matched};
  }
  auto first = torch::empty(
      {np}, torch::dtype(sizeof(F) == 4 ? torch::kInt32 : torch::kInt64)
                .device(dev));
  auto counts = torch::empty({np}, torch::dtype(torch::kInt32).device(dev));
  hipLaunchKernelGGL((join_probe_count_kernel<F, false>), grid, block, 0,
                     cur_stream(), a, mode, (F*)first.data_ptr(),
                     counts.data_ptr<int32_t>(), (bool*)nullptr);
  // int64 scan: offsets are incl[i] - counts[i], the total is the last entry
  auto incl = torch::cumsum(counts, 0, torch::kInt64);
  int64_t total = incl[np - 1].item<int64_t>();
  auto lidx = torch::empty({total}, opts64);
  auto ridx = torch::empty({total}, opts64);
  if (total > 0)
    hipLaunchKernelGGL(join_probe_fill_kernel<F>, grid, block, 0,
                       cur_stream(), a, (const F*)first.data_ptr(),
                       counts.data_ptr<int32_t>(), incl.data_ptr<int64_t>(),
                       lidx.data_ptr<int64_t>(), ridx.data_ptr<int64_t>(),
                       need_matched ? matched.data_ptr<bool>() : nullptr);
  return {lidx, ridx, matched};
}

// mode: 0=inner, 1=left, 2=semi, 3=anti.  matched (one bool per build row)
// is only filled when need_matched; otherwise it comes back empty.
std::vector<Tensor> join_probe(
    Tensor table, Tensor next, Tensor probe_hashes, Tensor build_hashes,
    const std::vector<int64_t>& tags_l, const std::vector<Tensor>& data_l,
    const std::vector<OptTensor>& off_l, const std::vector<OptTensor>& val_l,
    const std::vector<int64_t>& tags_r, const std::vector<Tensor>& data_r,
    const std::vector<OptTensor>& off_r, const std::vector<OptTensor>& val_r,
    int64_t mode, bool need_matched) {
  TORCH_CHECK(mode >= JOIN_INNER && mode <= JOIN_ANTI);
  int64_t nb = build_hashes.numel();
  auto pdescs = pack_descs(tags_l, data_l, off_l, val_l);
  auto bdescs = pack_descs(tags_r, data_r, off_r, val_r);
  ProbeArgs a{table.data_ptr<int64_t>(),
              next.data_ptr<int64_t>(),
              (const uint64_t*)probe_hashes.data_ptr<int64_t>(),
              (const uint64_t*)build_hashes.data_ptr<int64_t>(),
              (const ColDesc*)pdescs.data_ptr(),
              (const ColDesc*)bdescs.data_ptr(),
              (int)tags_l.size(),
              probe_hashes.numel(),
              (uint64_t)table.numel() - 1};
  auto dev = probe_hashes.device();
  if (nb < ((int64_t)1 << 31))
    return join_probe_t<int32_t>(a, (int)mode, nb, need_matched, dev);
  return join_probe_t<int64_t>(a, (int)mode, nb, need_matched, dev);
}
