// Fused expression evaluation for gfx950 (CDNA4): the interpreter.
//
// One kernel evaluates an entire projection / predicate list: a postfix
// program over (value f64, valid bool) stack slots, one thread per row,
// grid-stride.  It is the fallback for the hipRTC path (fusedjit.hip) and
// replaces chains of per-node torch elementwise kernels.
//
// The stack is f64.  The Python compiler (daft_amd/kernels/fused.py) only
// emits programs whose integer values provably stay within +-2^53, where
// f64 is exact; it bails on int64/uint64/timestamp columns.  OP_CAST rounds
// to f32 or wraps to a narrower integer width wherever the expression's
// dtype demands it.  Decimal(p<=18) columns are loaded as scaled int64 and
// DIVIDED by 10^scale (an exact f64 constant, so the quotient is correctly
// rounded; multiplying by the inexact 10^-scale is not).  AND/OR use Kleene
// three-valued logic matching kernels.logical_op.
#include "common.h"

#include "host_args.h"

using torch::Tensor;
using OptTensor = c10::optional<Tensor>;

namespace {

struct FCol {
  const void* data;
  const bool* valid;
  int64_t code;   // 0=f64 1=f32 2=i64 3=i32 4=i16 5=i8 6=bool/u8 7=u32 8=u64
  double scale;   // load divides by this (decimal 10^scale); 1.0 default
};

struct FOut {
  void* data;
  bool* valid;    // nullptr when statically all-valid
  int64_t code;   // 0=f64 1=f32 2=i64 3=i32 6=bool
  double scale;   // store divides by this (decimal rescale); 1.0 default
};

enum : int32_t {
  OP_COL = 0, OP_LIT = 1,
  OP_ADD = 2, OP_SUB = 3, OP_MUL = 4, OP_DIV = 5,
  OP_EQ = 6, OP_NE = 7, OP_LT = 8, OP_LE = 9, OP_GT = 10, OP_GE = 11,
  OP_AND = 12, OP_OR = 13, OP_NOT = 14, OP_NEG = 15,
  OP_ISNULL = 16, OP_NOTNULL = 17, OP_FILLNULL = 18, OP_SELECT = 19,
  OP_STORE = 20,
  OP_CAST = 21,   // arg: 1=f32 3=i32 4=i16 5=i8 6=u8 7=u32 9=bool 10=u16
};

#define FE_STACK 12

DEV_INLINE double fe_load(const FCol& c, int64_t i, bool* valid) {
  *valid = c.valid ? c.valid[i] : true;
  double v = 0.0;
  switch ((int)c.code) {
    case 0: v = ((const double*)c.data)[i]; break;
    case 1: v = (double)((const float*)c.data)[i]; break;
    case 2: v = (double)((const int64_t*)c.data)[i]; break;
    case 3: v = (double)((const int32_t*)c.data)[i]; break;
    case 4: v = (double)((const int16_t*)c.data)[i]; break;
    case 5: v = (double)((const int8_t*)c.data)[i]; break;
    case 6: v = (double)((const uint8_t*)c.data)[i]; break;
    case 7: v = (double)((const uint32_t*)c.data)[i]; break;
    case 8: v = (double)((const uint64_t*)c.data)[i]; break;
  }
  return v / c.scale;
}

// v is integral and within +-2^53 for the integer codes (compiler
// guarantee), so the int64 conversion is exact and the narrowing wraps.
DEV_INLINE double fe_cast(double v, int code) {
  switch (code) {
    case 1: return (double)(float)v;
    case 3: return (double)(int32_t)(int64_t)v;
    case 4: return (double)(int16_t)(int64_t)v;
    case 5: return (double)(int8_t)(int64_t)v;
    case 6: return (double)(uint8_t)(int64_t)v;
    case 7: return (double)(uint32_t)(int64_t)v;
    case 9: return v != 0.0 ? 1.0 : 0.0;
    case 10: return (double)(uint16_t)(int64_t)v;
  }
  return v;
}

template <bool HV>
__global__ void fused_eval_kernel(const int32_t* __restrict__ prog,
                                  int n_ins,
                                  const double* __restrict__ lits,
                                  int n_lits,
                                  const FCol* __restrict__ cols,
                                  const FOut* __restrict__ outs,
                                  int64_t n) {
  // 4 rows per thread, program walked once per 4-row vector: amortizes
  // instruction decode/branching 4x and keeps loads coalesced (row =
  // base + r*blockDim + tid).  Program + literals staged in LDS.
  constexpr int R = 4;
  constexpr int VSTACK = 8;
  extern __shared__ double smem[];
  double* slits = smem;
  int32_t* sprog = (int32_t*)(smem + n_lits);
  for (int t = threadIdx.x; t < n_lits; t += blockDim.x) slits[t] = lits[t];
  for (int t = threadIdx.x; t < n_ins * 2; t += blockDim.x)
    sprog[t] = prog[t];
  __syncthreads();

  const int64_t chunk = (int64_t)blockDim.x * R;
  const int64_t gstride = (int64_t)gridDim.x * chunk;
  for (int64_t base = (int64_t)blockIdx.x * chunk; base < n;
       base += gstride) {
    double st[VSTACK][R];
    bool va[VSTACK][R];
    const int64_t row0 = base + threadIdx.x;
    const bool full = base + chunk <= n;
    int sp = 0;
    for (int pc = 0; pc < n_ins; ++pc) {
      const int32_t op = sprog[pc * 2], arg = sprog[pc * 2 + 1];
      switch (op) {
        case OP_COL: {
          const FCol c = cols[arg];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int64_t i = row0 + (int64_t)r * blockDim.x;
            bool v = true;
            st[sp][r] = (full || i < n) ? fe_load(c, i, &v) : 0.0;
            if (HV) va[sp][r] = v;
          }
          ++sp;
        } break;
        case OP_LIT: {
          const double v = slits[arg];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            st[sp][r] = v;
            if (HV) va[sp][r] = true;
          }
          ++sp;
        } break;
#define FE_BIN(expr)                                                      \
  --sp;                                                                   \
  _Pragma("unroll") for (int r = 0; r < R; ++r) {                         \
    const double a = st[sp - 1][r], b = st[sp][r];                        \
    (void)a; (void)b;                                                     \
    st[sp - 1][r] = (expr);                                               \
    if (HV) va[sp - 1][r] = va[sp - 1][r] && va[sp][r];                   \
  }                                                                       \
  break;
        case OP_ADD: FE_BIN(a + b)
        case OP_SUB: FE_BIN(a - b)
        case OP_MUL: FE_BIN(a * b)
        case OP_DIV: FE_BIN(a / b)
        case OP_EQ: FE_BIN(a == b ? 1.0 : 0.0)
        case OP_NE: FE_BIN(a != b ? 1.0 : 0.0)
        case OP_LT: FE_BIN(a < b ? 1.0 : 0.0)
        case OP_LE: FE_BIN(a <= b ? 1.0 : 0.0)
        case OP_GT: FE_BIN(a > b ? 1.0 : 0.0)
        case OP_GE: FE_BIN(a >= b ? 1.0 : 0.0)
#undef FE_BIN
        case OP_AND: {
          --sp;
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const bool a = st[sp - 1][r] != 0.0, b = st[sp][r] != 0.0;
            st[sp - 1][r] = (a && b) ? 1.0 : 0.0;
            if (HV) {
              const bool av = va[sp - 1][r], bv = va[sp][r];
              va[sp - 1][r] = (av && bv) || (av && !a) || (bv && !b);
            }
          }
        } break;
        case OP_OR: {
          --sp;
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const bool a = st[sp - 1][r] != 0.0, b = st[sp][r] != 0.0;
            st[sp - 1][r] = (a || b) ? 1.0 : 0.0;
            if (HV) {
              const bool av = va[sp - 1][r], bv = va[sp][r];
              va[sp - 1][r] = (av && bv) || (av && a) || (bv && b);
            }
          }
        } break;
        case OP_NOT:
#pragma unroll
          for (int r = 0; r < R; ++r)
            st[sp - 1][r] = st[sp - 1][r] != 0.0 ? 0.0 : 1.0;
          break;
        case OP_NEG:
#pragma unroll
          for (int r = 0; r < R; ++r) st[sp - 1][r] = -st[sp - 1][r];
          break;
        case OP_CAST:
#pragma unroll
          for (int r = 0; r < R; ++r)
            st[sp - 1][r] = fe_cast(st[sp - 1][r], arg);
          break;
        case OP_ISNULL:
#pragma unroll
          for (int r = 0; r < R; ++r) {
            st[sp - 1][r] = (HV && !va[sp - 1][r]) ? 1.0 : 0.0;
            if (HV) va[sp - 1][r] = true;
          }
          break;
        case OP_NOTNULL:
#pragma unroll
          for (int r = 0; r < R; ++r) {
            st[sp - 1][r] = (!HV || va[sp - 1][r]) ? 1.0 : 0.0;
            if (HV) va[sp - 1][r] = true;
          }
          break;
        case OP_FILLNULL:
          --sp;
          if (HV) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
              if (!va[sp - 1][r]) {
                st[sp - 1][r] = st[sp][r];
                va[sp - 1][r] = va[sp][r];
              }
            }
          }
          break;
        case OP_SELECT: {
          sp -= 2;
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const bool m =
                (st[sp - 1][r] != 0.0) && (!HV || va[sp - 1][r]);
            st[sp - 1][r] = m ? st[sp][r] : st[sp + 1][r];
            if (HV) va[sp - 1][r] = m ? va[sp][r] : va[sp + 1][r];
          }
        } break;
        case OP_STORE: {
          --sp;
          const FOut o = outs[arg];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int64_t i = row0 + (int64_t)r * blockDim.x;
            if (!full && i >= n) continue;
            if (HV && o.valid) o.valid[i] = va[sp][r];
            const double v = st[sp][r] / o.scale;
            switch ((int)o.code) {
              case 0: ((double*)o.data)[i] = v; break;
              case 1: ((float*)o.data)[i] = (float)v; break;
              case 2: ((int64_t*)o.data)[i] = (int64_t)llrint(v); break;
              case 3: ((int32_t*)o.data)[i] = (int32_t)llrint(v); break;
              case 6: ((bool*)o.data)[i] = v != 0.0; break;
            }
          }
        } break;
      }
    }
  }
}

}  // namespace

std::vector<Tensor> fused_eval(Tensor prog, Tensor lits,
                               std::vector<Tensor> cols,
                               std::vector<OptTensor> valids,
                               std::vector<int64_t> codes,
                               std::vector<double> scales,
                               std::vector<int64_t> out_codes,
                               std::vector<double> out_scales,
                               std::vector<int64_t> out_need_valid,
                               int64_t n) {
  auto dev = cols.empty() ? prog.device() : cols[0].device();
  int ncols = (int)cols.size();
  int nouts = (int)out_codes.size();

  auto hc = torch::empty({ncols * 4}, torch::dtype(torch::kInt64));
  int64_t* h = hc.data_ptr<int64_t>();
  for (int i = 0; i < ncols; ++i) {
    h[i * 4 + 0] = (int64_t)cols[i].data_ptr();
    h[i * 4 + 1] =
        valids[i].has_value() ? (int64_t)valids[i]->data_ptr<bool>() : 0;
    h[i * 4 + 2] = codes[i];
    double s = scales[i];
    __builtin_memcpy(&h[i * 4 + 3], &s, 8);
  }
  auto dcols = ncols ? hc.to(dev) : hc;

  static const torch::ScalarType kOutTy[] = {
      torch::kFloat64, torch::kFloat32, torch::kInt64,
      torch::kInt32,   torch::kInt16,   torch::kInt8,
      torch::kBool};
  std::vector<Tensor> results;
  auto ho = torch::empty({nouts * 4}, torch::dtype(torch::kInt64));
  int64_t* ho_p = ho.data_ptr<int64_t>();
  for (int k = 0; k < nouts; ++k) {
    auto out = torch::empty({n}, torch::dtype(kOutTy[out_codes[k]])
                                     .device(dev));
    Tensor vout;
    bool nv = out_need_valid[k] != 0;
    if (nv) vout = torch::empty({n}, torch::dtype(torch::kBool).device(dev));
    ho_p[k * 4 + 0] = (int64_t)out.data_ptr();
    ho_p[k * 4 + 1] = nv ? (int64_t)vout.data_ptr<bool>() : 0;
    ho_p[k * 4 + 2] = out_codes[k];
    double s = out_scales[k];
    __builtin_memcpy(&ho_p[k * 4 + 3], &s, 8);
    results.push_back(out);
    results.push_back(nv ? vout : Tensor());
  }
  auto douts = ho.to(dev);
  auto dprog = prog.to(dev);
  auto dlits = lits.numel() ? lits.to(dev) : lits;

  if (n == 0) return results;
  bool has_valid = false;
  for (auto& v : valids)
    if (v.has_value()) has_valid = true;
  for (auto nv : out_need_valid)
    if (nv) has_valid = true;
  int block = 256;
  int n_ins = (int)(dprog.numel() / 2);
  int n_lits = (int)dlits.numel();
  size_t smem = sizeof(double) * n_lits + sizeof(int32_t) * n_ins * 2;
  int grid = grid_1d(n, block, /*items_per_thread=*/4);
  auto kern = has_valid ? fused_eval_kernel<true> : fused_eval_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(block), smem, cur_stream(),
                     (const int32_t*)dprog.data_ptr(), n_ins,
                     n_lits ? (const double*)dlits.data_ptr() : nullptr,
                     n_lits, (const FCol*)dcols.data_ptr(),
                     (const FOut*)douts.data_ptr(), n);
  return results;
}
