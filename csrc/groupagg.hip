// Grouped aggregation for gfx950: fold each row's value into the accumulator
// slot of its group.  A slot is 64 bits; what it holds for (type, op) is
// known only to the four slot_* functions below.  Low-cardinality shapes
// stage per-block partials in LDS (160 KiB/CU) and emit one global atomic
// per block per live slot; high-cardinality shapes go straight to global
// atomics (low contention).  Valid-row counters are u32 in LDS, i64 in HBM.

#include <type_traits>

#include "common.h"
#include "host_args.h"
#include "api.h"

// ---------------------------------------------------------------------------
// slot primitives.  f64 min/max slots hold order-encoded bits (unsigned
// integer order == IEEE total order: -NaN < -inf < -0.0 < +0.0 < +inf < NaN)
// so one u64 atomicMin/Max serves; sums hold the plain value.
// ---------------------------------------------------------------------------

DEV_INLINE uint64_t f64_order_bits(uint64_t b) {
  return (b & 0x8000000000000000ull) ? ~b : (b ^ 0x8000000000000000ull);
}
DEV_INLINE uint64_t f64_from_order_bits(uint64_t b) {
  return (b & 0x8000000000000000ull) ? (b ^ 0x8000000000000000ull) : ~b;
}

template <typename T>
constexpr bool kIsF64 = std::is_same<T, double>::value;

// identity of a slot
template <typename T>
__host__ __device__ inline uint64_t slot_identity(int op) {
  if (op == AGG_MIN) return kIsF64<T> ? ~0ull : (uint64_t)INT64_MAX;
  if (op == AGG_MAX) return kIsF64<T> ? 0ull : (uint64_t)INT64_MIN;
  return 0;  // sum (integer 0 and +0.0 share bits), count
}

// merge a partial slot (or an encoded value) into `dst`, LDS or global
template <typename T>
DEV_INLINE void slot_merge(uint64_t* dst, uint64_t part, int op) {
  if (op == AGG_SUM) {
    if constexpr (kIsF64<T>) {
      double v;
      __builtin_memcpy(&v, &part, 8);
      atomicAdd((double*)dst, v);
    } else {
      atomicAdd((unsigned long long*)dst, (unsigned long long)part);
    }
  } else if (op == AGG_MIN) {
    if constexpr (kIsF64<T>)
      atomicMin((unsigned long long*)dst, (unsigned long long)part);
    else
      atomicMin((long long*)dst, (long long)part);
  } else if (op == AGG_MAX) {
    if constexpr (kIsF64<T>)
      atomicMax((unsigned long long*)dst, (unsigned long long)part);
    else
      atomicMax((long long*)dst, (long long)part);
  }
}

// update a slot with one value
template <typename T>
DEV_INLINE void slot_update(uint64_t* dst, T v, int op) {
  uint64_t b;
  __builtin_memcpy(&b, &v, 8);
  if (kIsF64<T> && op != AGG_SUM) b = f64_order_bits(b);
  slot_merge<T>(dst, b, op);
}

// decode a finished slot; empty f64 min/max groups read 0.0 (cnt == 0 tells
// them apart), every other empty slot keeps its identity
template <typename T>
DEV_INLINE uint64_t slot_decode(uint64_t slot, int op, int64_t cnt) {
  if (kIsF64<T> && (op == AGG_MIN || op == AGG_MAX))
    return cnt > 0 ? f64_from_order_bits(slot) : 0ull;
  return slot;
}

DEV_INLINE void count_add(uint32_t* p, uint32_t k) { atomicAdd(p, k); }
DEV_INLINE void count_add(int64_t* p, uint64_t k) {
  atomicAdd((unsigned long long*)p, (unsigned long long)k);
}

// per-block LDS staging shared by both kernels; op_of(slot) names the op.
// Count slots have a counter and no accumulator.
template <typename T, typename OpOf>
DEV_INLINE void stage_init(uint64_t* lacc, uint32_t* lcnt, int64_t slots,
                           OpOf op_of) {
  for (int64_t s = threadIdx.x; s < slots; s += blockDim.x) {
    int op = op_of(s);
    if (op != AGG_COUNT) lacc[s] = slot_identity<T>(op);
    lcnt[s] = 0;
  }
  __syncthreads();
}

template <typename T, typename OpOf>
DEV_INLINE void stage_flush(const uint64_t* lacc, const uint32_t* lcnt,
                            int64_t slots, uint64_t* out, int64_t* cnt,
                            OpOf op_of) {
  __syncthreads();
  for (int64_t s = threadIdx.x; s < slots; s += blockDim.x) {
    if (lcnt[s] == 0) continue;
    count_add(&cnt[s], lcnt[s]);
    int op = op_of(s);
    if (op != AGG_COUNT) slot_merge<T>(&out[s], lacc[s], op);
  }
}

extern __shared__ char agg_smem[];

// ---------------------------------------------------------------------------
// single-column sum/min/max/count of f64 or i64 values
// ---------------------------------------------------------------------------

template <typename T, int OP, bool STAGED>
__global__ void grouped_agg_kernel(const int64_t* gids, const T* vals,
                                   const bool* valid, int64_t n,
                                   int64_t num_groups, uint64_t* out,
                                   int64_t* cnt) {
  constexpr bool kHasAcc = OP != AGG_COUNT;
  auto op_of = [](int64_t) { return OP; };
  uint64_t* lacc = (uint64_t*)agg_smem;
  uint32_t* lcnt =
      (uint32_t*)(agg_smem + (kHasAcc ? num_groups * sizeof(uint64_t) : 0));
  if constexpr (STAGED) stage_init<T>(lacc, lcnt, num_groups, op_of);
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    if (valid && !valid[i]) continue;
    int64_t g = gids[i];
    if constexpr (STAGED)
      count_add(&lcnt[g], 1u);
    else
      count_add(&cnt[g], 1ull);
    if constexpr (kHasAcc)
      slot_update<T>(STAGED ? &lacc[g] : &out[g], vals[i], OP);
  }
  if constexpr (STAGED)
    stage_flush<T>(lacc, lcnt, num_groups, out, cnt, op_of);
}

template <typename T>
__global__ void grouped_agg_decode_kernel(uint64_t* out, const int64_t* cnt,
                                          int64_t num_groups, int64_t slots,
                                          const MAggCol* cols, int op) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots;
       s += stride) {
    uint64_t raw = out[s];
    uint64_t v = slot_decode<T>(
        raw, cols ? (int)cols[s / num_groups].op : op, cnt[s]);
    if (v != raw) out[s] = v;
  }
}

static void launch_decode(Tensor out, Tensor cnt, int64_t num_groups,
                          const MAggCol* cols, int op) {
  int64_t slots = out.numel();
  if (slots == 0) return;
  hipLaunchKernelGGL(grouped_agg_decode_kernel<double>,
                     dim3(grid_1d(slots, 256)), dim3(256), 0, cur_stream(),
                     (uint64_t*)out.data_ptr<int64_t>(),
                     cnt.data_ptr<int64_t>(), num_groups, slots, cols, op);
}

// [is_f64][op][staged]; counting never reads values, one instantiation serves
#define AGG_VARIANTS(T, OP)                             \
  {(const void*)grouped_agg_kernel<T, OP, false>,       \
   (const void*)grouped_agg_kernel<T, OP, true>}
static const void* const kAggKernels[2][4][2] = {
    {AGG_VARIANTS(int64_t, AGG_SUM), AGG_VARIANTS(int64_t, AGG_MIN),
     AGG_VARIANTS(int64_t, AGG_MAX), AGG_VARIANTS(int64_t, AGG_COUNT)},
    {AGG_VARIANTS(double, AGG_SUM), AGG_VARIANTS(double, AGG_MIN),
     AGG_VARIANTS(double, AGG_MAX), AGG_VARIANTS(int64_t, AGG_COUNT)}};
#undef AGG_VARIANTS

std::vector<Tensor> grouped_agg(Tensor group_ids, int64_t num_groups,
                                Tensor values, Tensor valid, int64_t op) {
  TORCH_CHECK(op >= AGG_SUM && op <= AGG_COUNT, "grouped_agg: unknown op");
  auto opts64 = torch::dtype(torch::kInt64).device(group_ids.device());
  int64_t n = group_ids.numel();
  bool counting = op == AGG_COUNT;
  bool is_f64 = !counting && values.dtype() == torch::kFloat64;
  TORCH_CHECK(counting || is_f64 || values.dtype() == torch::kInt64,
              "grouped_agg expects f64/i64 working dtype");
  auto cnt = torch::zeros({num_groups}, opts64);
  Tensor out;
  if (!counting) {
    uint64_t id = is_f64 ? slot_identity<double>((int)op)
                         : slot_identity<int64_t>((int)op);
    out = torch::full({num_groups}, (int64_t)id, opts64);
  }
  if (n > 0) {
    // LDS budget: keep under 48 KiB/block for occupancy (160 KiB/CU on CDNA4)
    int64_t lds = num_groups * ((counting ? 0 : 8) + sizeof(uint32_t));
    bool staged = num_groups <= (counting ? 8192 : 4096) && lds <= 48 * 1024;
    const int64_t* g = group_ids.data_ptr<int64_t>();
    const void* v = counting ? nullptr : values.data_ptr();
    const bool* vp = (valid.defined() && valid.numel() > 0)
                         ? valid.data_ptr<bool>() : nullptr;
    int64_t* o = counting ? nullptr : out.data_ptr<int64_t>();
    int64_t* c = cnt.data_ptr<int64_t>();
    void* args[] = {&g, &v, &vp, &n, &num_groups, &o, &c};
    int block = 256;
    HIP_CHECK(hipLaunchKernel(kAggKernels[is_f64][op][staged],
                              dim3(grid_1d(n, block, staged ? 8 : 1)),
                              dim3(block), args, staged ? lds : 0,
                              cur_stream()));
  }
  if (is_f64) {
    if (op != AGG_SUM) launch_decode(out, cnt, num_groups, nullptr, (int)op);
    out = out.view(torch::kFloat64);
  }
  return {out, cnt};
}

Tensor grouped_count(Tensor group_ids, int64_t num_groups, Tensor valid) {
  return grouped_agg(group_ids, num_groups, Tensor(), valid, AGG_COUNT)[1];
}

// ---------------------------------------------------------------------------
// fused multi-aggregate: ONE pass over (gids, value columns) computing every
// f64 sum/min/max/count of an aggregation at once.  The per-agg path reads
// gids once per aggregate (600M x 8B x n_aggs on a Q1-shaped plan); here
// gids load once per row.  Capability of the reference's per-type agg
// kernels (daft-core/src/array/ops/{sum,mean,count,compare_agg}.rs) fused
// the MI355X way.  Slot of (agg a, group g) is a * num_groups + g.
// ---------------------------------------------------------------------------

template <bool STAGED>
__global__ void grouped_multi_agg_kernel(const int64_t* gids, int64_t n,
                                         int64_t num_groups, int n_aggs,
                                         const MAggCol* cols, uint64_t* out,
                                         int64_t* cnt) {
  // staged slots fit 32 bits (<= 2048): keep their index math narrow
  using Idx = std::conditional_t<STAGED, int, int64_t>;
  auto op_of = [=](int64_t s) {
    return (int)cols[(Idx)s / (Idx)num_groups].op;
  };
  Idx slots = (Idx)num_groups * n_aggs;
  uint64_t* lacc = (uint64_t*)agg_smem;
  uint32_t* lcnt = (uint32_t*)(agg_smem + (size_t)slots * sizeof(uint64_t));
  if constexpr (STAGED) stage_init<double>(lacc, lcnt, slots, op_of);
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    Idx g = (Idx)gids[i];
#pragma unroll 1
    for (int a = 0; a < n_aggs; ++a) {
      MAggCol c = cols[a];
      if (c.valid && !c.valid[i]) continue;
      Idx s = (Idx)a * (Idx)num_groups + g;
      if constexpr (STAGED)
        count_add(&lcnt[s], 1u);
      else
        count_add(&cnt[s], 1ull);
      if (c.op != AGG_COUNT)
        slot_update<double>(STAGED ? &lacc[s] : &out[s], c.data[i],
                            (int)c.op);
    }
  }
  if constexpr (STAGED)
    stage_flush<double>(lacc, lcnt, slots, out, cnt, op_of);
}

std::vector<Tensor> grouped_multi_agg(Tensor gids, int64_t num_groups,
                                      std::vector<Tensor> datas,
                                      std::vector<OptTensor> valids,
                                      std::vector<int64_t> ops) {
  auto dev = gids.device();
  int n_aggs = (int)ops.size();
  int64_t n = gids.numel();
  int64_t slots = num_groups * n_aggs;
  // pack MAggCol descriptors; slots start at their op's identity
  auto host = torch::empty({n_aggs * 3}, torch::dtype(torch::kInt64));
  auto out = torch::zeros({slots}, torch::dtype(torch::kInt64).device(dev));
  int64_t* h = host.data_ptr<int64_t>();
  for (int i = 0; i < n_aggs; ++i) {
    h[i * 3 + 0] = datas[i].defined() && datas[i].numel()
                       ? (int64_t)datas[i].data_ptr<double>() : 0;
    h[i * 3 + 1] = valids[i].has_value()
                       ? (int64_t)valids[i]->data_ptr<bool>() : 0;
    h[i * 3 + 2] = ops[i];
    if (int64_t id = (int64_t)slot_identity<double>((int)ops[i]))
      out.slice(0, i * num_groups, (i + 1) * num_groups).fill_(id);
  }
  auto descs = host.to(dev);
  const MAggCol* cols = (const MAggCol*)descs.data_ptr();
  auto cnt = torch::zeros({slots}, torch::dtype(torch::kInt64).device(dev));
  if (n > 0) {
    int block = 256;
    if (slots <= 2048) {  // accumulators fit LDS
      size_t lds = (size_t)slots * (sizeof(uint64_t) + sizeof(uint32_t));
      hipLaunchKernelGGL(grouped_multi_agg_kernel<true>,
                         dim3(grid_1d(n, block, 8)), dim3(block), lds,
                         cur_stream(), gids.data_ptr<int64_t>(), n, num_groups,
                         n_aggs, cols, (uint64_t*)out.data_ptr<int64_t>(),
                         cnt.data_ptr<int64_t>());
    } else {  // slot contention is negligible; the win is reading gids once
      hipLaunchKernelGGL(grouped_multi_agg_kernel<false>,
                         dim3(grid_1d(n, block, 4)), dim3(block), 0,
                         cur_stream(), gids.data_ptr<int64_t>(), n, num_groups,
                         n_aggs, cols, (uint64_t*)out.data_ptr<int64_t>(),
                         cnt.data_ptr<int64_t>());
    }
  }
  launch_decode(out, cnt, num_groups, cols, 0);
  return {out.view(torch::kFloat64), cnt};
}
