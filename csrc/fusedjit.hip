// hipRTC-backed JIT for fused expression kernels (gfx950).
//
// The generic interpreter (fusedexpr.hip) pays for its dynamically
// indexed stack with scratch traffic; a projection list compiled to
// straight-line code runs at memory bandwidth.  Python generates the
// kernel source per (expression list, schema, validity pattern) and this
// launcher compiles it ONCE per process (cache keyed by source) with
// hipRTC, then launches through the module API.  Column/output buffers
// travel via the same packed descriptor arrays as the interpreter, so a
// cached kernel is reusable across batches and steps.
#include "common.h"

#include "host_args.h"
#include "api.h"
#include <hip/hiprtc.h>

#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

using torch::Tensor;
using OptTensor = c10::optional<Tensor>;

namespace {

struct JitEntry {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  hipFunction_t fn2 = nullptr;  // second kernel of the module, if it has one
};

std::unordered_map<std::string, JitEntry>& jit_cache() {
  static std::unordered_map<std::string, JitEntry> c;
  return c;
}
std::mutex g_jit_mu;

JitEntry compile_or_get(const std::string& src, const char* name = "fe",
                        const char* name2 = nullptr) {
  std::lock_guard<std::mutex> lk(g_jit_mu);
  auto& cache = jit_cache();
  auto it = cache.find(src);
  if (it != cache.end()) {
    if (it->second.fn == nullptr)
      throw std::runtime_error("fused jit: compile previously failed");
    return it->second;
  }

  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), "fe.hip", 0, nullptr,
                          nullptr) != HIPRTC_SUCCESS)
    throw std::runtime_error("hiprtcCreateProgram failed");
  const char* opts[] = {"--offload-arch=gfx950", "-O3"};
  hiprtcResult rc = hiprtcCompileProgram(prog, 2, opts);
  if (rc != HIPRTC_SUCCESS) {
    size_t log_size = 0;
    hiprtcGetProgramLogSize(prog, &log_size);
    std::string log(log_size, '\0');
    hiprtcGetProgramLog(prog, log.data());
    hiprtcDestroyProgram(&prog);
    // cache the failure: retrying an impossible compile per batch would
    // cost ~150 ms every call
    cache.emplace(src, JitEntry{});
    throw std::runtime_error("hiprtc compile failed:\n" + log);
  }
  size_t code_size = 0;
  hiprtcGetCodeSize(prog, &code_size);
  std::vector<char> code(code_size);
  hiprtcGetCode(prog, code.data());
  hiprtcDestroyProgram(&prog);

  JitEntry e;
  if (hipModuleLoadData(&e.mod, code.data()) != hipSuccess)
    throw std::runtime_error("hipModuleLoadData failed");
  if (hipModuleGetFunction(&e.fn, e.mod, name) != hipSuccess ||
      (name2 && hipModuleGetFunction(&e.fn2, e.mod, name2) != hipSuccess))
    throw std::runtime_error(std::string("hipModuleGetFunction(") + name +
                             ") failed");
  cache.emplace(src, e);
  return e;
}

}  // namespace

bool fused_jit_available() {
  return true;
}

std::vector<Tensor> fused_eval_jit(const std::string& src,
                                   std::vector<Tensor> cols,
                                   std::vector<OptTensor> valids,
                                   std::vector<int64_t> out_codes,
                                   std::vector<int64_t> out_need_valid,
                                   int64_t n) {
  auto dev = cols.empty() ? torch::Device(torch::kCUDA, 0)
                          : cols[0].device();
  int ncols = (int)cols.size();
  int nouts = (int)out_codes.size();

  // pack column descriptors {data, valid} (dtype/scale are baked into the
  // generated source)
  auto hc = torch::empty({std::max(ncols, 1) * 2},
                         torch::dtype(torch::kInt64));
  int64_t* h = hc.data_ptr<int64_t>();
  for (int i = 0; i < ncols; ++i) {
    h[i * 2 + 0] = (int64_t)cols[i].data_ptr();
    h[i * 2 + 1] =
        valids[i].has_value() ? (int64_t)valids[i]->data_ptr<bool>() : 0;
  }
  auto dcols = hc.to(dev);

  static const torch::ScalarType kOutTy[] = {
      torch::kFloat64, torch::kFloat32, torch::kInt64,
      torch::kInt32,   torch::kInt16,   torch::kInt8,
      torch::kBool};
  std::vector<Tensor> results;
  auto ho = torch::empty({std::max(nouts, 1) * 2},
                         torch::dtype(torch::kInt64));
  int64_t* ho_p = ho.data_ptr<int64_t>();
  for (int k = 0; k < nouts; ++k) {
    auto out = torch::empty({n},
                            torch::dtype(kOutTy[out_codes[k]]).device(dev));
    Tensor vout;
    bool nv = out_need_valid[k] != 0;
    if (nv) vout = torch::empty({n}, torch::dtype(torch::kBool).device(dev));
    ho_p[k * 2 + 0] = (int64_t)out.data_ptr();
    ho_p[k * 2 + 1] = nv ? (int64_t)vout.data_ptr<bool>() : 0;
    results.push_back(out);
    results.push_back(nv ? vout : Tensor());
  }
  auto douts = ho.to(dev);
  if (n == 0) return results;

  hipFunction_t fn = compile_or_get(src).fn;
  void* cols_p = (void*)dcols.data_ptr();
  void* outs_p = (void*)douts.data_ptr();
  long long nn = (long long)n;
  void* params[] = {&cols_p, &outs_p, &nn};
  int block = 256;
  int grid = grid_1d(n, block, /*items_per_thread=*/2);
  hipStream_t stream = cur_stream();
  hipError_t rc = hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, 0,
                                        stream, params, nullptr);
  if (rc != hipSuccess)
    throw std::runtime_error(std::string("fused jit launch failed: ") +
                             hipGetErrorString(rc));
  return results;
}

// ---------------------------------------------------------------------------
// Filter -> Aggregate over a few groups in ONE pass: the generated row body
// evaluates the predicate, the group slot and every aggregate input in
// registers, and the skeleton below folds them.  Slot of (accumulator a,
// group g) is a * G + g and the slot encodings are groupagg.hip's (restated
// here: the text is compiled by hipRTC and cannot include a project header):
// order-encoded bits for f64 min/max, plain f64 for sums, u32 counters in
// LDS and i64 in HBM.  One global atomic per live slot per block.
//
// Contention.  Up to kAggRegSlots slots (q1: 6 x 6, q6: 1) every thread
// keeps its own partials in registers, selected by comparing the slot with
// each group, and touches LDS once, after its last row: a handful of hot
// slots would serialise a wave's LDS atomics 64 deep on every row.  Above
// that the rows of a wave spread over many slots and plain LDS atomics do,
// as in grouped_multi_agg_kernel.
// ---------------------------------------------------------------------------
namespace {

constexpr int64_t kAggMaxSlots = 2048;  // grouped_multi_agg's staging bound
constexpr int64_t kAggMaxAccs = 16;     // accumulator loops are unrolled
constexpr int64_t kAggRegSlots = 48;    // register partials up to here

// In front of this text the launcher defines FA_A, FA_G, FA_REG and the
// tables fa_op[FA_A] (AggOp) and fa_own[FA_A] (1: the input can be null, so
// the accumulator counts its own rows; 0: its count is the group's hits).
const char* const kAggHead = R"K(
// a product must round before it is summed, as when it was materialised
#pragma clang fp contract(off)
typedef unsigned long long fa_u64;
enum { FA_SUM = 0, FA_MIN = 1, FA_MAX = 2, FA_COUNT = 3 };
#define FA_SLOTS (FA_A * FA_G)
#define FA_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define FA_DEV __HIP_MEMORY_SCOPE_AGENT

// unsigned order of the encoded bits == IEEE total order
// (-NaN < -inf < -0.0 < +0.0 < +inf < NaN)
__device__ inline __attribute__((always_inline)) fa_u64 fa_order_bits(double v) {
  const fa_u64 b = __builtin_bit_cast(fa_u64, v);
  return (b >> 63) ? ~b : (b ^ 0x8000000000000000ull);
}
__device__ inline __attribute__((always_inline)) fa_u64 fa_from_order_bits(fa_u64 b) {
  return (b >> 63) ? (b ^ 0x8000000000000000ull) : ~b;
}
__device__ constexpr fa_u64 fa_identity(int op) {
  return op == FA_MIN ? ~0ull : 0ull;   // max: lowest bits; sum: +0.0
}
// what a slot holds for one value
__device__ inline __attribute__((always_inline)) fa_u64 fa_encode(double v, int op) {
  return op == FA_SUM ? __builtin_bit_cast(fa_u64, v) : fa_order_bits(v);
}
// merge a partial slot (or an encoded value) into dst, LDS or global
template <int SCOPE>
__device__ inline __attribute__((always_inline)) void fa_merge(fa_u64* dst, fa_u64 part, int op) {
  if (op == FA_SUM)
    __hip_atomic_fetch_add((double*)dst, __builtin_bit_cast(double, part),
                           __ATOMIC_RELAXED, SCOPE);
  else if (op == FA_MIN)
    __hip_atomic_fetch_min(dst, part, __ATOMIC_RELAXED, SCOPE);
  else if (op == FA_MAX)
    __hip_atomic_fetch_max(dst, part, __ATOMIC_RELAXED, SCOPE);
}

extern "C" __global__ void __launch_bounds__(256)
fa(const long long* __restrict__ cols, fa_u64* __restrict__ acc,
   long long* __restrict__ cnt, long long* __restrict__ hit, long long n) {
)K";

// after the hoisted column pointers: staging, accumulators, row loop
const char* const kAggLoop = R"K(
  __shared__ fa_u64 lacc[FA_SLOTS];
  __shared__ unsigned int lcnt[FA_SLOTS + FA_G];   // own counts, then hits
#pragma unroll
  for (int a = 0; a < FA_A; ++a)
    for (int g = threadIdx.x; g < FA_G; g += blockDim.x) {
      lacc[a * FA_G + g] = fa_identity(fa_op[a]);
      lcnt[a * FA_G + g] = 0;
    }
  for (int g = threadIdx.x; g < FA_G; g += blockDim.x) lcnt[FA_SLOTS + g] = 0;
  __syncthreads();
#if FA_REG
  double rsum[FA_A][FA_G];
  fa_u64 rext[FA_A][FA_G];
  unsigned int rcnt[FA_A + 1][FA_G];
#pragma unroll
  for (int g = 0; g < FA_G; ++g) {
    rcnt[FA_A][g] = 0;
#pragma unroll
    for (int a = 0; a < FA_A; ++a) {
      rsum[a][g] = 0.0;
      rext[a][g] = fa_identity(fa_op[a]);
      rcnt[a][g] = 0;
    }
  }
#endif
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
)K";

// after the row body, which has defined: bool fa_pass, int fa_slot,
// double fa_v[FA_A], bool fa_ok[FA_A]
const char* const kAggTail = R"K(
#if FA_REG
#pragma unroll
    for (int g = 0; g < FA_G; ++g) {
      const bool m = fa_pass && fa_slot == g;
      rcnt[FA_A][g] += m;
#pragma unroll
      for (int a = 0; a < FA_A; ++a) {
        const bool ok = m && fa_ok[a];
        if (fa_own[a]) rcnt[a][g] += ok;
        if (fa_op[a] == FA_SUM) {
          if (ok) rsum[a][g] += fa_v[a];
        } else if (fa_op[a] != FA_COUNT) {
          const fa_u64 b = fa_order_bits(fa_v[a]);
          if (ok && (fa_op[a] == FA_MIN ? b < rext[a][g] : b > rext[a][g]))
            rext[a][g] = b;
        }
      }
    }
#else
    // a code outside its vocabulary must not index past the staging
    if (fa_pass && (unsigned int)fa_slot < (unsigned int)FA_G) {
      __hip_atomic_fetch_add(&lcnt[FA_SLOTS + fa_slot], 1u, __ATOMIC_RELAXED,
                             FA_WG);
#pragma unroll
      for (int a = 0; a < FA_A; ++a) {
        if (!fa_ok[a]) continue;
        const int s = a * FA_G + fa_slot;
        if (fa_own[a])
          __hip_atomic_fetch_add(&lcnt[s], 1u, __ATOMIC_RELAXED, FA_WG);
        if (fa_op[a] != FA_COUNT)
          fa_merge<FA_WG>(&lacc[s], fa_encode(fa_v[a], fa_op[a]), fa_op[a]);
      }
    }
#endif
  }
#if FA_REG
  // each thread's partials go to the block's staging once
#pragma unroll
  for (int g = 0; g < FA_G; ++g) {
    if (rcnt[FA_A][g] == 0) continue;
    __hip_atomic_fetch_add(&lcnt[FA_SLOTS + g], rcnt[FA_A][g],
                           __ATOMIC_RELAXED, FA_WG);
#pragma unroll
    for (int a = 0; a < FA_A; ++a) {
      const int s = a * FA_G + g;
      if (fa_own[a]) {
        if (rcnt[a][g] == 0) continue;
        __hip_atomic_fetch_add(&lcnt[s], rcnt[a][g], __ATOMIC_RELAXED, FA_WG);
      }
      if (fa_op[a] == FA_SUM)
        fa_merge<FA_WG>(&lacc[s], __builtin_bit_cast(fa_u64, rsum[a][g]),
                        FA_SUM);
      else if (fa_op[a] != FA_COUNT)
        fa_merge<FA_WG>(&lacc[s], rext[a][g], fa_op[a]);
    }
  }
#endif
  __syncthreads();
  // one global atomic per live slot per block
#pragma unroll
  for (int a = 0; a < FA_A; ++a)
    for (int g = threadIdx.x; g < FA_G; g += blockDim.x) {
      const int s = a * FA_G + g;
      const unsigned int c = fa_own[a] ? lcnt[s] : lcnt[FA_SLOTS + g];
      if (c == 0) continue;
      __hip_atomic_fetch_add((fa_u64*)&cnt[s], (fa_u64)c, __ATOMIC_RELAXED,
                             FA_DEV);
      if (fa_op[a] != FA_COUNT) fa_merge<FA_DEV>(&acc[s], lacc[s], fa_op[a]);
    }
  for (int g = threadIdx.x; g < FA_G; g += blockDim.x)
    if (lcnt[FA_SLOTS + g])
      __hip_atomic_fetch_add((fa_u64*)&hit[g], (fa_u64)lcnt[FA_SLOTS + g],
                             __ATOMIC_RELAXED, FA_DEV);
}

// min/max slots leave as f64; an empty one reads 0.0 (cnt == 0 tells)
extern "C" __global__ void fa_decode(fa_u64* __restrict__ acc,
                                     const long long* __restrict__ cnt) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= FA_SLOTS) return;
  bool ext = false;
#pragma unroll
  for (int a = 0; a < FA_A; ++a)
    if (fa_op[a] == FA_MIN || fa_op[a] == FA_MAX) ext |= s / FA_G == a;
  if (ext) acc[s] = cnt[s] > 0 ? fa_from_order_bits(acc[s]) : 0ull;
}
)K";

void check_agg_shape(const std::vector<int64_t>& ops,
                     const std::vector<int64_t>& own_valid, int64_t groups) {
  int64_t a = (int64_t)ops.size();
  TORCH_CHECK(a >= 1 && a <= kAggMaxAccs, "fused_agg: 1..", kAggMaxAccs,
              " accumulators, got ", a);
  TORCH_CHECK(own_valid.size() == ops.size(),
              "fused_agg: own_valid must have one entry per accumulator");
  TORCH_CHECK(groups >= 1 && a * groups <= kAggMaxSlots,
              "fused_agg: accumulators x groups must be in 1..", kAggMaxSlots);
  for (int64_t op : ops)
    TORCH_CHECK(op >= AGG_SUM && op <= AGG_COUNT, "fused_agg: unknown op ",
                op);
}

std::string int_table(const char* name, const std::vector<int64_t>& v) {
  std::string s = std::string("__device__ const int ") + name + "[" +
                  std::to_string(v.size()) + "] = {";
  for (size_t i = 0; i < v.size(); ++i)
    s += (i ? ", " : "") + std::to_string(v[i]);
  return s + "};\n";
}

}  // namespace

std::string fused_agg_source(const std::string& body,
                             std::vector<int64_t> col_has_valid,
                             std::vector<int64_t> ops,
                             std::vector<int64_t> own_valid, int64_t groups) {
  check_agg_shape(ops, own_valid, groups);
  for (auto& o : own_valid) o = o != 0;
  int64_t a = (int64_t)ops.size();
  std::string s;
  s += "#define FA_A " + std::to_string(a) + "\n";
  s += "#define FA_G " + std::to_string(groups) + "\n";
  s += "#define FA_REG " +
       std::to_string(a * groups <= kAggRegSlots ? 1 : 0) + "\n";
  s += int_table("fa_op", ops);
  s += int_table("fa_own", own_valid);
  s += kAggHead;
  for (size_t ix = 0; ix < col_has_valid.size(); ++ix) {
    std::string k = std::to_string(ix);
    s += "  const void* C" + k + "d = (const void*)cols[" + k + " * 2];\n";
    if (col_has_valid[ix])
      s += "  const bool* C" + k + "v = (const bool*)cols[" + k +
           " * 2 + 1];\n";
  }
  s += kAggLoop;
  s += body;
  s += kAggTail;
  return s;
}

std::vector<Tensor> fused_agg_jit(const std::string& body,
                                  std::vector<Tensor> cols,
                                  std::vector<OptTensor> valids,
                                  std::vector<int64_t> ops,
                                  std::vector<int64_t> own_valid,
                                  int64_t groups, int64_t n) {
  const char* who = "fused_agg_jit";
  TORCH_CHECK(!cols.empty() && cols.size() == valids.size(), who,
              ": one validity entry per column, at least one column");
  TORCH_CHECK(n >= 0, who, ": n must not be negative");
  auto dev = cols[0].device();
  TORCH_CHECK(dev.is_cuda(), who, ": columns must be on a GPU device");
  std::vector<int64_t> col_has_valid;
  int ncols = (int)cols.size();
  auto hc = torch::empty({ncols * 2}, torch::dtype(torch::kInt64));
  int64_t* h = hc.data_ptr<int64_t>();
  for (int i = 0; i < ncols; ++i) {
    TORCH_CHECK(cols[i].device() == dev && cols[i].is_contiguous() &&
                    cols[i].dim() == 1 && cols[i].numel() == n,
                who, ": column ", i, " must be contiguous [", n, "] on ", dev);
    const bool* v = check_valid(who, valids[i], n, dev);
    h[i * 2 + 0] = (int64_t)cols[i].data_ptr();
    h[i * 2 + 1] = (int64_t)v;
    col_has_valid.push_back(v != nullptr);
  }
  std::string src =
      fused_agg_source(body, col_has_valid, ops, own_valid, groups);

  // one buffer: acc[A*G] | cnt[A*G] | hit[G]; min slots start at all-ones
  int64_t a = (int64_t)ops.size(), slots = a * groups;
  auto buf = torch::zeros({2 * slots + groups},
                          torch::dtype(torch::kInt64).device(dev));
  Tensor acc = buf.slice(0, 0, slots), cnt = buf.slice(0, slots, 2 * slots),
         hit = buf.slice(0, 2 * slots);
  bool any_ext = false;
  for (int64_t i = 0; i < a; ++i) {
    any_ext |= ops[i] == AGG_MIN || ops[i] == AGG_MAX;
    if (ops[i] == AGG_MIN)
      acc.slice(0, i * groups, (i + 1) * groups).fill_(-1);
  }
  if (n > 0) {
    auto dcols = hc.to(dev);
    JitEntry e = compile_or_get(src, "fa", "fa_decode");
    int scratch = 0;
    if (hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES,
                            e.fn) == hipSuccess)
      TORCH_CHECK(scratch == 0, who, ": kernel spills ", scratch,
                  " B of scratch per lane");
    void* cols_p = (void*)dcols.data_ptr();
    void* acc_p = acc.data_ptr();
    void* cnt_p = cnt.data_ptr();
    void* hit_p = hit.data_ptr();
    long long nn = (long long)n;
    void* params[] = {&cols_p, &acc_p, &cnt_p, &hit_p, &nn};
    hipStream_t stream = cur_stream();
    HIP_CHECK(hipModuleLaunchKernel(e.fn, grid_1d(n, 256, 8), 1, 1, 256, 1, 1,
                                    0, stream, params, nullptr));
    if (any_ext) {
      void* dparams[] = {&acc_p, &cnt_p};
      HIP_CHECK(hipModuleLaunchKernel(e.fn2, grid_1d(slots, 256), 1, 1, 256,
                                      1, 1, 0, stream, dparams, nullptr));
    }
  } else if (any_ext) {
    acc.zero_();
  }
  return {acc.view(torch::kFloat64), cnt, hit};
}
