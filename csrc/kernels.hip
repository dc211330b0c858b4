// Core row-wise HIP kernels for gfx950: row hashing, stream compaction,
// string gather, hash groupby, hash partitioning (grouped aggregation lives
// in groupagg.hip, joins in join.hip).  MI355X-native design notes:
//  * one thread per row, grid-stride, grids capped at 8 blocks/CU
//  * hash tables are power-of-2 bucket arrays in HBM; inserts use one
//    device-scope atomic each (no locks) — per-XCD L2 non-coherence is safe
//    because all cross-workgroup communication is via atomics
//  * low-cardinality aggregations stage per-block accumulators in LDS
//    (160 KiB/CU) and emit one global atomic per block per group
#include "common.h"
#include "host_args.h"
#include "row_ops.h"
#include "api.h"

// ---------------------------------------------------------------------------
// descriptor packing
// ---------------------------------------------------------------------------

Tensor pack_descs(const std::vector<int64_t>& tags,
                  const std::vector<Tensor>& datas,
                  const std::vector<OptTensor>& offsets,
                  const std::vector<OptTensor>& validities) {
  int n = (int)tags.size();
  auto host = torch::empty({n * 4}, torch::dtype(torch::kInt64));
  int64_t* h = host.data_ptr<int64_t>();
  for (int i = 0; i < n; ++i) {
    h[i * 4 + 0] = (int64_t)datas[i].data_ptr();
    h[i * 4 + 1] = offsets[i].has_value()
                       ? (int64_t)offsets[i]->data_ptr<int64_t>()
                       : 0;
    h[i * 4 + 2] = validities[i].has_value()
                       ? (int64_t)validities[i]->data_ptr<bool>()
                       : 0;
    h[i * 4 + 3] = tags[i];
  }
  return host.to(datas[0].device(), /*non_blocking=*/false);
}

// ---------------------------------------------------------------------------
// row hashing
// ---------------------------------------------------------------------------

__global__ void hash_rows_kernel(const ColDesc* cols, int ncols, int64_t n,
                                 uint64_t seed, uint64_t* out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    out[i] = row_hash(cols, ncols, i, seed);
  }
}

Tensor hash_rows(const std::vector<int64_t>& tags,
                 const std::vector<Tensor>& datas,
                 const std::vector<OptTensor>& offsets,
                 const std::vector<OptTensor>& validities, int64_t n,
                 int64_t seed) {
  auto descs = pack_descs(tags, datas, offsets, validities);
  auto out = torch::empty({n}, torch::dtype(torch::kInt64)
                                   .device(datas[0].device()));
  if (n == 0) return out;
  int block = 256;
  hipLaunchKernelGGL(hash_rows_kernel, dim3(grid_1d(n, block)), dim3(block),
                     0, cur_stream(), (const ColDesc*)descs.data_ptr(),
                     (int)tags.size(), n, (uint64_t)seed,
                     (uint64_t*)out.data_ptr<int64_t>());
  return out;
}

// ---------------------------------------------------------------------------
// stream compaction: bool mask -> selected indices
// (ballot + wave prefix within block, block offsets via device cumsum)
// ---------------------------------------------------------------------------

__global__ void block_count_kernel(const bool* mask, int64_t n,
                                   int64_t chunk, int32_t* counts) {
  int64_t begin = (int64_t)blockIdx.x * chunk;
  int64_t end = min(begin + chunk, n);
  int32_t local = 0;
  for (int64_t i = begin + threadIdx.x; i < end; i += blockDim.x)
    local += mask[i] ? 1 : 0;
  __shared__ int32_t acc;
  if (threadIdx.x == 0) acc = 0;
  __syncthreads();
  // wave reduce then one atomic per wave
  for (int off = WAVE / 2; off; off >>= 1)
    local += __shfl_down(local, off, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) atomicAdd(&acc, local);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = acc;
}

__global__ void compact_kernel(const bool* mask, int64_t n, int64_t chunk,
                               const int32_t* block_offsets, int64_t* out) {
  int64_t begin = (int64_t)blockIdx.x * chunk;
  int64_t end = min(begin + chunk, n);
  __shared__ int64_t base;
  __shared__ int32_t wave_counts[256 / WAVE];
  if (threadIdx.x == 0) base = block_offsets[blockIdx.x];
  __syncthreads();
  int lane = threadIdx.x & (WAVE - 1);
  int wid = threadIdx.x / WAVE;
  int nwaves = blockDim.x / WAVE;
  for (int64_t tile = begin; tile < end; tile += blockDim.x) {
    int64_t i = tile + threadIdx.x;
    bool sel = i < end && mask[i];
    uint64_t ballot = __ballot(sel);
    int rank = __popcll(ballot & ((1ull << lane) - 1));
    int wtotal = __popcll(ballot);
    if (lane == 0) wave_counts[wid] = wtotal;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wid; ++w) woff += wave_counts[w];
    if (sel) out[base + woff + rank] = i;
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int w = 0; w < nwaves; ++w) t += wave_counts[w];
      base += t;
    }
    __syncthreads();
  }
}

Tensor compact_indices(Tensor mask) {
  TORCH_CHECK(mask.is_cuda() && mask.dtype() == torch::kBool);
  mask = mask.contiguous();
  int64_t n = mask.numel();
  auto dev = mask.device();
  if (n == 0) return torch::empty({0}, torch::dtype(torch::kInt64).device(dev));
  int block = 256;
  int64_t chunk = (n + kMaxBlocks - 1) / kMaxBlocks;
  if (chunk < block) chunk = block;
  int nblocks = (int)((n + chunk - 1) / chunk);
  auto counts = torch::empty({nblocks},
                             torch::dtype(torch::kInt32).device(dev));
  hipLaunchKernelGGL(block_count_kernel, dim3(nblocks), dim3(block), 0,
                     cur_stream(), mask.data_ptr<bool>(), n, chunk,
                     counts.data_ptr<int32_t>());
  auto offs = torch::cumsum(counts, 0, torch::kInt32) - counts;
  auto total_t = counts.sum();
  int64_t total = total_t.item<int64_t>();
  auto out = torch::empty({total}, torch::dtype(torch::kInt64).device(dev));
  if (total == 0) return out;
  hipLaunchKernelGGL(compact_kernel, dim3(nblocks), dim3(block), 0,
                     cur_stream(), mask.data_ptr<bool>(), n, chunk,
                     offs.contiguous().data_ptr<int32_t>(),
                     out.data_ptr<int64_t>());
  return out;
}

// ---------------------------------------------------------------------------
// string gather: one thread per OUTPUT BYTE (coalesced writes; row lookup via
// binary search over output offsets, L2/LDS-friendly)
// ---------------------------------------------------------------------------

DEV_INLINE int64_t upper_bound_row(const int64_t* offs, int64_t nrows,
                                   int64_t j) {
  int64_t lo = 0, hi = nrows;  // offs has nrows+1 entries; find row of byte j
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (offs[mid + 1] <= j)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// One thread per output byte j: f(j, row, within) writes the byte that lies
// `within` bytes into output row `row`.  One binary search per 256-byte block
// (LDS-shared), then threads walk offsets linearly — offsets are monotone so
// the walk is short and the reads coalesce within the block.
template <typename F>
__global__ void out_bytes_kernel(const int64_t* out_off, int64_t nrows,
                                 int64_t total, F f) {
  __shared__ int64_t block_row;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j0 = (int64_t)blockIdx.x * blockDim.x; j0 < total;
       j0 += stride) {
    if (threadIdx.x == 0) block_row = upper_bound_row(out_off, nrows, j0);
    __syncthreads();
    int64_t j = j0 + threadIdx.x;
    if (j < total) {
      int64_t row = block_row;
      while (out_off[row + 1] <= j) ++row;
      f(j, row, j - out_off[row]);
    }
    __syncthreads();
  }
}

template <typename F>
static void launch_out_bytes(Tensor out_off, int64_t nrows, int64_t total,
                             F f) {
  int block = 256;
  hipLaunchKernelGGL(out_bytes_kernel<F>, dim3(grid_1d(total, block)),
                     dim3(block), 0, cur_stream(),
                     out_off.data_ptr<int64_t>(), nrows, total, f);
}

struct GatherBytes {  // out row r is source row idx[r]
  const int64_t* src_off;
  const uint8_t* src_bytes;
  const int64_t* idx;
  uint8_t* out;
  DEV_INLINE void operator()(int64_t j, int64_t row, int64_t within) const {
    out[j] = src_bytes[src_off[idx[row]] + within];
  }
};

std::vector<Tensor> take_string(Tensor offsets, Tensor bytes, Tensor idx) {
  StrCol c = check_strcol("take_string", offsets, bytes);
  check_tensor("take_string", "idx", idx, torch::kInt64, offsets.device());
  TORCH_CHECK(idx.dim() == 1, "take_string: idx must be 1-d");
  auto lens = offsets.slice(0, 1) - offsets.slice(0, 0, c.n);
  auto [out_off, total] = offsets_from_lens(lens.index_select(0, idx));
  auto out = torch::empty({total}, bytes.options());
  if (total > 0)
    launch_out_bytes(out_off, idx.numel(), total,
                     GatherBytes{c.offs, c.bytes, idx.data_ptr<int64_t>(),
                                 out.data_ptr<uint8_t>()});
  return {out_off, out};
}

struct MergeStrings {  // out row r is t's row r where m[r], else f's
  const bool* m;
  const int64_t* t_off;
  const uint8_t* t_bytes;
  const int64_t* f_off;
  const uint8_t* f_bytes;
  uint8_t* out;
  DEV_INLINE void operator()(int64_t j, int64_t row, int64_t within) const {
    out[j] = m[row] ? t_bytes[t_off[row] + within]
                    : f_bytes[f_off[row] + within];
  }
};

Tensor merge_strings(Tensor mask, Tensor t_off, Tensor t_bytes, Tensor f_off,
                     Tensor f_bytes, Tensor out_off) {
  StrCol t = check_strcol("merge_strings", t_off, t_bytes);
  auto dev = t_off.device();
  StrCol f = check_strcol_rows("merge_strings", f_off, f_bytes, t.n, dev);
  check_tensor("merge_strings", "mask", mask, torch::kBool, dev);
  TORCH_CHECK(mask.numel() == t.n, "merge_strings: mask must have ", t.n,
              " rows");
  check_tensor("merge_strings", "out_off", out_off, torch::kInt64, dev);
  TORCH_CHECK(out_off.dim() == 1 && out_off.numel() == t.n + 1,
              "merge_strings: out_off must have ", t.n + 1, " entries");
  int64_t total = t.n > 0 ? out_off[t.n].item<int64_t>() : 0;
  auto out = torch::empty({total}, t_bytes.options());
  if (total > 0)
    launch_out_bytes(out_off, t.n, total,
                     MergeStrings{mask.data_ptr<bool>(), t.offs, t.bytes, f.offs, f.bytes,
                                  out.data_ptr<uint8_t>()});
  return out;
}

// ---------------------------------------------------------------------------
// hash groupby: open-addressing insert keyed by row hash with full key verify
// (ref semantics: daft-recordbatch probe_table.rs; GPU design: linear-probe
// table of owner row indices, dense ids assigned by atomic counter)
// ---------------------------------------------------------------------------

// Linear-probe from row i's home slot until it either claims an empty slot
// (returns true: i is the first sighting of its key) or finds a slot whose
// owner row equals it (returns false).  *slot_out is that slot.
DEV_INLINE bool claim_or_find(const uint64_t* hashes, const ColDesc* cols,
                              int ncols, int64_t i, int64_t* table,
                              uint64_t mask, uint64_t* slot_out) {
  uint64_t h = hashes[i];
  uint64_t slot = h & mask;
  bool claimed;
  while (true) {
    // Plain read first: slots transition -1 -> owner exactly once, so a
    // non-(-1) read is final; a stale -1 is corrected by the device-scope
    // CAS below.  This avoids serializing 10^8 CAS ops on a handful of
    // slots for low-cardinality groupbys (the Q1 shape).
    long long prev = table[slot];
    if (prev == -1ll) {
      prev = atomicCAS((unsigned long long*)&table[slot],
                       (unsigned long long)(-1ll), (unsigned long long)i);
      if (prev == -1ll) {
        claimed = true;
        break;
      }
    }
    if (hashes[prev] == h &&
        row_eq(cols, cols, ncols, prev, i, /*null_eq=*/true)) {
      claimed = false;
      break;
    }
    slot = (slot + 1) & mask;
  }
  *slot_out = slot;
  return claimed;
}

__global__ void groupby_insert_kernel(const uint64_t* hashes,
                                      const ColDesc* cols, int ncols,
                                      int64_t n, int64_t* table,
                                      uint64_t mask, int64_t* row_slot) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    uint64_t slot;
    claim_or_find(hashes, cols, ncols, i, table, mask, &slot);
    row_slot[i] = (int64_t)slot;
  }
}

__global__ void groupby_assign_ids_kernel(const int64_t* table,
                                          const int64_t* row_slot, int64_t n,
                                          int32_t* slot_gid, int64_t* reps,
                                          int32_t* counter) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t slot = row_slot[i];
    if (table[slot] == i) {
      int32_t gid = atomicAdd(counter, 1);
      slot_gid[slot] = gid;
      reps[gid] = i;
    }
  }
}

__global__ void groupby_gather_ids_kernel(const int64_t* row_slot,
                                          const int32_t* slot_gid, int64_t n,
                                          int64_t* gids) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    gids[i] = (int64_t)slot_gid[row_slot[i]];
}

std::vector<Tensor> groupby(Tensor hashes, const std::vector<int64_t>& tags,
                            const std::vector<Tensor>& datas,
                            const std::vector<OptTensor>& offsets,
                            const std::vector<OptTensor>& validities) {
  auto dev = hashes.device();
  int64_t n = hashes.numel();
  auto opts64 = torch::dtype(torch::kInt64).device(dev);
  if (n == 0) {
    return {torch::empty({0}, opts64), torch::empty({0}, opts64)};
  }
  auto descs = pack_descs(tags, datas, offsets, validities);
  int64_t cap = table_capacity(n);
  auto table = torch::full({cap}, -1, opts64);
  auto row_slot = torch::empty({n}, opts64);
  int block = 256;
  hipLaunchKernelGGL(groupby_insert_kernel, dim3(grid_1d(n, block)),
                     dim3(block), 0, cur_stream(),
                     (const uint64_t*)hashes.data_ptr<int64_t>(),
                     (const ColDesc*)descs.data_ptr(), (int)tags.size(), n,
                     table.data_ptr<int64_t>(), (uint64_t)(cap - 1),
                     row_slot.data_ptr<int64_t>());
  auto slot_gid = torch::empty({cap}, torch::dtype(torch::kInt32).device(dev));
  auto reps_full = torch::empty({n}, opts64);
  auto counter = torch::zeros({1}, torch::dtype(torch::kInt32).device(dev));
  hipLaunchKernelGGL(groupby_assign_ids_kernel, dim3(grid_1d(n, block)),
                     dim3(block), 0, cur_stream(), table.data_ptr<int64_t>(),
                     row_slot.data_ptr<int64_t>(), n,
                     slot_gid.data_ptr<int32_t>(),
                     reps_full.data_ptr<int64_t>(),
                     counter.data_ptr<int32_t>());
  auto gids = torch::empty({n}, opts64);
  hipLaunchKernelGGL(groupby_gather_ids_kernel, dim3(grid_1d(n, block)),
                     dim3(block), 0, cur_stream(),
                     row_slot.data_ptr<int64_t>(),
                     slot_gid.data_ptr<int32_t>(), n,
                     gids.data_ptr<int64_t>());
  int64_t num_groups = counter.item<int32_t>();
  return {gids, reps_full.slice(0, 0, num_groups)};
}

// one-pass count-distinct: insert (group, value) pairs into an
// open-addressing table; the CAS winner (first sighting of a distinct pair)
// increments its group's counter.  No dense ids / rep gathers needed.
__global__ void count_distinct_kernel(const uint64_t* hashes,
                                      const ColDesc* cols, int ncols,
                                      const int64_t* gids, int64_t n,
                                      int64_t* table, uint64_t mask,
                                      int64_t* cnt) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    if (row_has_null(cols, ncols, i)) continue;  // nulls don't count
    uint64_t slot;
    if (claim_or_find(hashes, cols, ncols, i, table, mask, &slot))
      atomicAdd((unsigned long long*)&cnt[gids[i]], 1ull);
  }
}

Tensor count_distinct_pairs(Tensor hashes, const std::vector<int64_t>& tags,
                            const std::vector<Tensor>& datas,
                            const std::vector<OptTensor>& offsets,
                            const std::vector<OptTensor>& validities,
                            Tensor gids, int64_t num_groups) {
  auto dev = hashes.device();
  int64_t n = hashes.numel();
  auto cnt = torch::zeros({num_groups},
                          torch::dtype(torch::kInt64).device(dev));
  if (n == 0) return cnt;
  auto descs = pack_descs(tags, datas, offsets, validities);
  int64_t cap = table_capacity(n);
  auto table = torch::full({cap}, -1,
                           torch::dtype(torch::kInt64).device(dev));
  int block = 256;
  hipLaunchKernelGGL(count_distinct_kernel, dim3(grid_1d(n, block)),
                     dim3(block), 0, cur_stream(),
                     (const uint64_t*)hashes.data_ptr<int64_t>(),
                     (const ColDesc*)descs.data_ptr(), (int)tags.size(),
                     gids.data_ptr<int64_t>(), n,
                     table.data_ptr<int64_t>(), (uint64_t)(cap - 1),
                     cnt.data_ptr<int64_t>());
  return cnt;
}

// dense-range groupby support: first-occurrence index per packed key
// (LDS-staged atomicMin for small ranges — global atomics on a handful of
// addresses would serialize)
__global__ void dense_first_lds_kernel(const int64_t* packed, int64_t n,
                                       int64_t rng, int64_t* first) {
  extern __shared__ uint32_t lmin[];
  for (int64_t g = threadIdx.x; g < rng; g += blockDim.x)
    lmin[g] = 0xFFFFFFFFu;
  __syncthreads();
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    atomicMin(&lmin[packed[i]], (uint32_t)i);
  __syncthreads();
  for (int64_t g = threadIdx.x; g < rng; g += blockDim.x)
    if (lmin[g] != 0xFFFFFFFFu)
      atomicMin((unsigned long long*)&first[g],
                (unsigned long long)lmin[g]);
}

__global__ void dense_first_global_kernel(const int64_t* packed, int64_t n,
                                          int64_t* first) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    atomicMin((unsigned long long*)&first[packed[i]],
              (unsigned long long)i);
}

Tensor dense_first_index(Tensor packed, int64_t rng, int64_t sentinel) {
  auto dev = packed.device();
  int64_t n = packed.numel();
  auto first = torch::full({rng}, sentinel,
                           torch::dtype(torch::kInt64).device(dev));
  if (n == 0) return first;
  TORCH_CHECK(n < (int64_t)0xFFFFFFFF, "dense_first_index: n must fit u32");
  int block = 256;
  int64_t lds = rng * sizeof(uint32_t);
  if (rng <= 8192 && lds <= 48 * 1024) {
    hipLaunchKernelGGL(dense_first_lds_kernel, dim3(grid_1d(n, block, 8)),
                       dim3(block), lds, cur_stream(),
                       packed.data_ptr<int64_t>(), n, rng,
                       first.data_ptr<int64_t>());
  } else {
    hipLaunchKernelGGL(dense_first_global_kernel,
                       dim3(grid_1d(n, block)), dim3(block), 0, cur_stream(),
                       packed.data_ptr<int64_t>(), n,
                       first.data_ptr<int64_t>());
  }
  return first;
}

// ---------------------------------------------------------------------------
// partition helper
// ---------------------------------------------------------------------------

__global__ void u64_mod_kernel(const uint64_t* h, int64_t n, uint64_t d,
                               int64_t* out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    out[i] = (int64_t)(h[i] % d);
}

Tensor u64_mod(Tensor hashes, int64_t n_partitions) {
  int64_t n = hashes.numel();
  auto out = torch::empty({n}, hashes.options());
  if (n > 0) {
    int block = 256;
    hipLaunchKernelGGL(u64_mod_kernel, dim3(grid_1d(n, block)), dim3(block),
                       0, cur_stream(),
                       (const uint64_t*)hashes.data_ptr<int64_t>(), n,
                       (uint64_t)n_partitions, out.data_ptr<int64_t>());
  }
  return out;
}
