// As-of join probe (gfx950): for every left row, one binary search inside the
// row's `by` group of the sorted right side, then a pick by strategy.
//
// Layout.  Keys on both sides are order-preserving u64 bit patterns
// (rowops._order_key_u64), so every compare is one unsigned 64-bit compare
// whatever the column type was.  The right side arrives filtered to usable
// rows and stably sorted by (group, key); group g owns the sorted positions
// [seg_offsets[g], seg_offsets[g + 1]) and right_rows[p] names the original
// right row at sorted position p.
//
// One thread per left row, 256-thread blocks, grid-stride.  The search is a
// chain of log2(segment length) dependent loads per row.  Nothing is staged
// in LDS: neighbouring lanes generally search different segments, so a tile
// of the right side has no reuse inside a block; the top levels of each
// segment's search tree stay in L2 instead.  Reads of the left side and the
// output store are coalesced; the loop body is predicated (`?:`), so lanes
// of a wave diverge only on trip count.  All positions are int64.
#include "common.h"
#include "host_args.h"
#include "api.h"

constexpr int ASOF_BLOCK = 256;
constexpr uint64_t ASOF_SIGN = 0x8000000000000000ull;

enum AsofStrategy : int { ASOF_BACKWARD = 0, ASOF_FORWARD = 1, ASOF_NEAREST = 2 };

// inverse of the float branch of _order_key_u64
DEV_INLINE double asof_decode_f64(uint64_t e) {
  uint64_t bits = (e & ASOF_SIGN) ? (e ^ ASOF_SIGN) : ~e;
  return __longlong_as_double((long long)bits);
}

// Is the forward candidate (key f >= pivot) at least as near as the backward
// one (key b < pivot)?  A tie goes forward, to the larger key.
DEV_INLINE bool asof_forward_wins(uint64_t key, uint64_t f, uint64_t b,
                                  bool float_keys) {
  if (!float_keys) return f - key <= key - b;  // exact: x + 2^63 mod 2^64
  if (f == key) return true;                   // exact match, distance 0
  double p = asof_decode_f64(key);
  double df = fabs(asof_decode_f64(f) - p);
  double db = fabs(asof_decode_f64(b) - p);
  // a NaN distance counts as greatest, and equals another NaN distance
  bool nf = df != df, nb = db != db;
  if (nf || nb) return nb;
  return df <= db;
}

__global__ __launch_bounds__(ASOF_BLOCK) void asof_probe_kernel(
    const uint64_t* __restrict__ left_keys, const int64_t* __restrict__ left_gids,
    const uint64_t* __restrict__ right_keys,
    const int64_t* __restrict__ right_rows,
    const int64_t* __restrict__ seg_offsets, int64_t nl, int64_t m,
    int64_t num_groups, int strategy, bool allow_exact, bool float_keys,
    int64_t* __restrict__ out) {
  // backward wants the end of the run of equal keys, forward its start;
  // !allow_exact swaps them.  Nearest always searches for the start.
  const bool upper = strategy == ASOF_BACKWARD
                         ? allow_exact
                         : (strategy == ASOF_FORWARD ? !allow_exact : false);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nl;
       i += stride) {
    int64_t g = left_gids[i];
    int64_t res = -1;
    if (g >= 0 && g < num_groups) {
      // the wrapper guarantees monotone offsets within [0, m]; the clamp
      // keeps a broken caller from reading outside right_keys
      int64_t a = max(seg_offsets[g], (int64_t)0);
      int64_t b = min(seg_offsets[g + 1], m);
      if (a < b) {
        uint64_t key = left_keys[i];
        int64_t lo = a, hi = b;
        while (lo < hi) {
          int64_t mid = lo + ((hi - lo) >> 1);
          uint64_t v = right_keys[mid];
          bool go_right = upper ? v <= key : v < key;
          lo = go_right ? mid + 1 : lo;
          hi = go_right ? hi : mid;
        }
        int64_t pos = -1;
        if (strategy == ASOF_BACKWARD) {
          if (lo - 1 >= a) pos = lo - 1;
        } else if (strategy == ASOF_FORWARD) {
          if (lo < b) pos = lo;
        } else {
          bool has_f = lo < b, has_b = lo - 1 >= a;
          if (has_f && has_b)
            pos = asof_forward_wins(key, right_keys[lo], right_keys[lo - 1],
                                    float_keys)
                      ? lo
                      : lo - 1;
          else
            pos = has_f ? lo : lo - 1;  // a < b: one of them exists
        }
        if (pos >= 0) res = right_rows[pos];
      }
    }
    out[i] = res;
  }
}

Tensor asof_probe(Tensor left_keys, Tensor left_gids, Tensor right_keys,
                  Tensor right_rows, Tensor seg_offsets, int64_t strategy,
                  bool allow_exact, bool float_keys) {
  const char* who = "asof_probe";
  TORCH_CHECK(left_keys.is_cuda(), who, ": left_keys must be on a GPU device");
  auto dev = left_keys.device();
  check_tensor(who, "left_keys", left_keys, torch::kInt64, dev);
  check_tensor(who, "left_gids", left_gids, torch::kInt64, dev);
  check_tensor(who, "right_keys", right_keys, torch::kInt64, dev);
  check_tensor(who, "right_rows", right_rows, torch::kInt64, dev);
  check_tensor(who, "seg_offsets", seg_offsets, torch::kInt64, dev);
  TORCH_CHECK(left_keys.dim() == 1 && left_gids.dim() == 1 &&
                  right_keys.dim() == 1 && right_rows.dim() == 1 &&
                  seg_offsets.dim() == 1,
              who, ": every argument must be 1-D");
  TORCH_CHECK(left_gids.numel() == left_keys.numel(), who,
              ": left_gids must have ", left_keys.numel(), " rows, got ",
              left_gids.numel());
  TORCH_CHECK(right_rows.numel() == right_keys.numel(), who,
              ": right_rows must have ", right_keys.numel(), " rows, got ",
              right_rows.numel());
  TORCH_CHECK(seg_offsets.numel() >= 1, who,
              ": seg_offsets must hold num_groups + 1 entries");
  TORCH_CHECK(strategy >= ASOF_BACKWARD && strategy <= ASOF_NEAREST, who,
              ": strategy must be 0 (backward), 1 (forward) or 2 (nearest), "
              "got ", strategy);
  TORCH_CHECK(strategy != ASOF_NEAREST || allow_exact, who,
              ": nearest needs allow_exact");

  int64_t nl = left_keys.numel();
  auto out = torch::empty({nl}, torch::dtype(torch::kInt64).device(dev));
  if (nl == 0) return out;
  hipLaunchKernelGGL(
      asof_probe_kernel, dim3(grid_1d(nl, ASOF_BLOCK)), dim3(ASOF_BLOCK), 0,
      cur_stream(), (const uint64_t*)left_keys.data_ptr<int64_t>(),
      left_gids.data_ptr<int64_t>(),
      (const uint64_t*)right_keys.data_ptr<int64_t>(),
      right_rows.data_ptr<int64_t>(), seg_offsets.data_ptr<int64_t>(), nl,
      right_keys.numel(), seg_offsets.numel() - 1, (int)strategy, allow_exact,
      float_keys, out.data_ptr<int64_t>());
  return out;
}
