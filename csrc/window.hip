// Framed window aggregates (gfx950): segmented scans plus one lookup kernel.
//
// Sorted space.  run_window sorts rows by (partition id, order keys); sorted
// position p holds original row perm[p] and partition g owns the positions
// [seg_offsets[g], seg_offsets[g + 1]), as in asof.hip.  Values and validity
// stay in original row order: the scan gathers them through perm and the
// lookup scatters its outputs back through perm.
//
// Scan.  A state holds only what the op needs ({cnt}, {cnt, sum},
// {cnt, sum, sumsq}, {cnt, extreme}); a null input is the identity.  The
// combine is the segmented operator (f1,s1)+(f2,s2) = (f1|f2, f2 ? s2 :
// s1 op s2) with a head flag where a partition starts (forward) or ends
// (backward), and, for a sliding frame of width w, also at every multiple of
// w.  A backward scan is the forward algorithm over q = n - 1 - p, so tiles,
// aggregates and carries are all in q; only loads and stores map q to p.
//
// Three launches per scan, none waiting on another block:
//   A  one 256-thread block per tile of WIN_TILE positions.  A thread scans
//      WIN_ITEMS consecutive positions in registers, the 64 lane totals are
//      scanned with wave shuffles, the four wave totals cross through LDS.
//      Writes the tile-local inclusive scan, the tile's aggregate and the
//      offset of the tile's first head (WIN_TILE when it has none).
//   B  one block scans the tile aggregates, 256 per trip, into a carry-in
//      per tile.
//   C  folds the carry-in into the positions before each tile's first head.
//
// Lookup.  With F the forward and B the backward scan, a frame [lo, hi]
// (clamped to the partition) is F[hi] when lo is unbounded, B[lo] when hi is,
// and otherwise the van Herk / Gil-Werman pair over w-blocks, w = the frame
// width: B[lo] + F[hi] when lo and hi lie in different blocks, else whichever
// of the two covers exactly [lo, hi].  Nothing is subtracted, so a sliding
// float sum never cancels and min/max need no table.  All positions are
// int64.
#include <limits>

#include "common.h"
#include "host_args.h"
#include "api.h"

// no packed-fp32 instructions in this file's kernels (they hold none today:
// every value is a double or an int64)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

constexpr int WIN_BLOCK = 256;
constexpr int WIN_ITEMS = 4;
constexpr int WIN_TILE = WIN_BLOCK * WIN_ITEMS;  // 1024 positions per tile
constexpr int WIN_WAVES = WIN_BLOCK / WAVE;

enum WinOp : int {
  WIN_SUM = 0, WIN_COUNT = 1, WIN_MEAN = 2, WIN_MIN = 3, WIN_MAX = 4,
  WIN_VAR = 5, WIN_STDDEV = 6
};
enum WinBound : int { WIN_UNBOUNDED = 0, WIN_OFFSET = 1, WIN_PEER_END = 2 };

DEV_INLINE int64_t win_bits(double x) { return __double_as_longlong(x); }
DEV_INLINE int64_t win_bits(int64_t x) { return x; }
DEV_INLINE int64_t win_shfl_up(int64_t x, int d) {
  return (int64_t)__shfl_up((long long)x, d);
}
DEV_INLINE double win_shfl_up(double x, int d) { return __shfl_up(x, d); }

// ---------------------------------------------------------------------------
// states
// ---------------------------------------------------------------------------
struct CntState {
  int64_t cnt;
  static DEV_INLINE CntState identity() { return {0}; }
  template <class V>
  static DEV_INLINE CntState make(V) { return {1}; }
  static DEV_INLINE CntState combine(const CntState& a, const CntState& b) {
    return {a.cnt + b.cnt};
  }
  DEV_INLINE CntState shfl_up(int d) const { return {win_shfl_up(cnt, d)}; }
  DEV_INLINE int64_t result_bits(int) const { return cnt; }
};

template <class V>
struct SumState {
  int64_t cnt;
  V sum;
  static DEV_INLINE SumState identity() { return {0, V(0)}; }
  static DEV_INLINE SumState make(V v) { return {1, v}; }
  static DEV_INLINE SumState combine(const SumState& a, const SumState& b) {
    return {a.cnt + b.cnt, a.sum + b.sum};
  }
  DEV_INLINE SumState shfl_up(int d) const {
    return {win_shfl_up(cnt, d), win_shfl_up(sum, d)};
  }
  DEV_INLINE int64_t result_bits(int op) const {
    if (op == WIN_MEAN) return win_bits((double)sum / (double)cnt);
    return win_bits(sum);
  }
};

struct VarState {
  int64_t cnt;
  double sum, sumsq;
  static DEV_INLINE VarState identity() { return {0, 0.0, 0.0}; }
  template <class V>
  static DEV_INLINE VarState make(V v) {
    double x = (double)v;
    return {1, x, x * x};
  }
  static DEV_INLINE VarState combine(const VarState& a, const VarState& b) {
    return {a.cnt + b.cnt, a.sum + b.sum, a.sumsq + b.sumsq};
  }
  DEV_INLINE VarState shfl_up(int d) const {
    return {win_shfl_up(cnt, d), win_shfl_up(sum, d), win_shfl_up(sumsq, d)};
  }
  // population variance, sumsq/cnt - mean^2 clamped at 0
  DEV_INLINE int64_t result_bits(int op) const {
    double c = (double)cnt;
    double mean = sum / c;
    double var = fmax(sumsq / c - mean * mean, 0.0);
    return win_bits(op == WIN_STDDEV ? sqrt(var) : var);
  }
};

template <class V, bool IS_MAX>
struct ExtState {
  int64_t cnt;
  V ext;
  static DEV_INLINE ExtState identity() {
    if (std::numeric_limits<V>::has_infinity)
      return {0, IS_MAX ? -std::numeric_limits<V>::infinity()
                        : std::numeric_limits<V>::infinity()};
    return {0, IS_MAX ? std::numeric_limits<V>::lowest()
                      : std::numeric_limits<V>::max()};
  }
  static DEV_INLINE ExtState make(V v) { return {1, v}; }
  // a NaN on either side wins, as in torch.minimum / torch.maximum
  static DEV_INLINE ExtState combine(const ExtState& a, const ExtState& b) {
    V e;
    if (a.ext != a.ext) e = a.ext;
    else if (b.ext != b.ext) e = b.ext;
    else e = IS_MAX ? (a.ext < b.ext ? b.ext : a.ext)
                    : (b.ext < a.ext ? b.ext : a.ext);
    return {a.cnt + b.cnt, e};
  }
  DEV_INLINE ExtState shfl_up(int d) const {
    return {win_shfl_up(cnt, d), win_shfl_up(ext, d)};
  }
  DEV_INLINE int64_t result_bits(int) const { return win_bits(ext); }
};
using PeerState = ExtState<int64_t, false>;

// (f_prev, s_prev) + (f, s), in place on the later operand
template <class S>
DEV_INLINE void win_seg_combine(bool& f, S& s, bool f_prev, const S& s_prev) {
  if (!f) s = S::combine(s_prev, s);
  f |= f_prev;
}

// ---------------------------------------------------------------------------
// sorted-space geometry and sources
// ---------------------------------------------------------------------------
struct WinSeg {
  const int64_t* perm;
  const int64_t* gids;
  const int64_t* seg;
  int64_t n;
  int64_t num_groups;
};

// Original row and inclusive partition bounds of sorted position p.  The
// wrapper guarantees a permutation, gids below num_groups and monotone
// offsets from 0 to n; the clamps keep a broken caller inside the buffers.
DEV_INLINE void win_bounds(const WinSeg& sg, int64_t p, int64_t& row,
                           int64_t& ps, int64_t& pe) {
  row = min(max(sg.perm[p], (int64_t)0), sg.n - 1);
  int64_t g = min(max(sg.gids[row], (int64_t)0), sg.num_groups - 1);
  ps = min(max(sg.seg[g], (int64_t)0), p);
  pe = max(min(sg.seg[g + 1] - 1, sg.n - 1), p);
}

// values through perm; heads at partition edges and, for w > 0, w-blocks
template <class S, class V, bool FWD>
struct WinValueSrc {
  WinSeg sg;
  const V* values;    // original row order; null for a pure count
  const bool* valid;  // original row order; null when every row is valid
  int64_t w;
  DEV_INLINE void operator()(int64_t p, S& s, bool& head) const {
    int64_t row, ps, pe;
    win_bounds(sg, p, row, ps, pe);
    if (FWD) head = p == ps || (w > 0 && p % w == 0);
    else head = p == pe || (w > 0 && p % w == w - 1);
    if (!valid || valid[row]) s = S::make(values ? values[row] : V(0));
  }
};

// backward min over "p is the last row of its peer run ? p : +inf": the
// scan value at p is the end of p's peer run
struct WinPeerSrc {
  WinSeg sg;
  const bool* new_peer;  // sorted space: a new peer run starts here
  DEV_INLINE void operator()(int64_t p, PeerState& s, bool& head) const {
    int64_t row, ps, pe;
    win_bounds(sg, p, row, ps, pe);
    head = p == pe;
    if (head || new_peer[p + 1]) s = PeerState::make(p);
  }
};

// ---------------------------------------------------------------------------
// scan kernels
// ---------------------------------------------------------------------------
// Exclusive segmented scan of one (f, s) per thread across the block, and the
// block total.  Ends on a barrier, so the LDS arrays can be reused at once.
template <class S>
DEV_INLINE void win_block_exclusive(bool f, S s, bool& ef, S& es, bool& tf,
                                    S& ts, S* lds_s, int* lds_f) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    bool f2 = __shfl_up((int)f, d) != 0;
    S s2 = s.shfl_up(d);
    if (lane >= d) win_seg_combine(f, s, f2, s2);
  }
  if (lane == WAVE - 1) {
    lds_s[wave] = s;
    lds_f[wave] = f;
  }
  bool pf = __shfl_up((int)f, 1) != 0;
  S ps = s.shfl_up(1);
  if (lane == 0) {
    pf = false;
    ps = S::identity();
  }
  __syncthreads();
  ef = false;
  es = S::identity();
  tf = false;
  ts = S::identity();
#pragma unroll
  for (int w = 0; w < WIN_WAVES; ++w) {
    if (w == wave) {
      ef = tf;
      es = ts;
    }
    bool f2 = lds_f[w] != 0;
    S s2 = lds_s[w];
    win_seg_combine(f2, s2, tf, ts);
    tf = f2;
    ts = s2;
  }
  win_seg_combine(pf, ps, ef, es);
  ef = pf;
  es = ps;
  __syncthreads();
}

template <bool FWD>
DEV_INLINE int64_t win_pos(int64_t q, int64_t n) {
  return FWD ? q : n - 1 - q;
}

// A: tile-local inclusive scan, tile aggregate, offset of the first head
template <class S, bool FWD, class Src>
__global__ __launch_bounds__(WIN_BLOCK) void win_scan_tiles(
    Src src, int64_t n, S* __restrict__ out, S* __restrict__ tile_state,
    int* __restrict__ tile_first) {
  __shared__ S lds_s[WIN_WAVES];
  __shared__ int lds_f[WIN_WAVES];
  __shared__ int first_head;
  if (threadIdx.x == 0) first_head = WIN_TILE;
  __syncthreads();
  const int k0 = threadIdx.x * WIN_ITEMS;
  const int64_t q0 = (int64_t)blockIdx.x * WIN_TILE + k0;
  S x[WIN_ITEMS];
  bool hf[WIN_ITEMS];
  S acc = S::identity();
  bool f = false;
  int my_first = WIN_TILE;
#pragma unroll
  for (int i = 0; i < WIN_ITEMS; ++i) {
    S s = S::identity();
    bool h = false;
    if (q0 + i < n) src(win_pos<FWD>(q0 + i, n), s, h);
    if (h) {
      acc = s;
      if (!f) my_first = k0 + i;
      f = true;
    } else {
      acc = S::combine(acc, s);
    }
    x[i] = acc;
    hf[i] = f;
  }
  if (my_first < WIN_TILE) atomicMin(&first_head, my_first);
  bool ef, tf;
  S es, ts;
  win_block_exclusive(f, acc, ef, es, tf, ts, lds_s, lds_f);
#pragma unroll
  for (int i = 0; i < WIN_ITEMS; ++i)
    if (q0 + i < n)
      out[win_pos<FWD>(q0 + i, n)] = hf[i] ? x[i] : S::combine(es, x[i]);
  if (threadIdx.x == 0) {
    tile_state[blockIdx.x] = ts;
    tile_first[blockIdx.x] = first_head;
  }
}

// B: carry[j] = what flows into tile j from the tiles before it
template <class S>
__global__ __launch_bounds__(WIN_BLOCK) void win_scan_carries(
    const S* __restrict__ tile_state, const int* __restrict__ tile_first,
    int64_t ntiles, S* __restrict__ carry) {
  __shared__ S lds_s[WIN_WAVES];
  __shared__ int lds_f[WIN_WAVES];
  S run = S::identity();  // state since the last head, same in every thread
  for (int64_t base = 0; base < ntiles; base += WIN_BLOCK) {
    int64_t j = base + threadIdx.x;
    bool f = false;
    S s = S::identity();
    if (j < ntiles) {
      s = tile_state[j];
      f = tile_first[j] < WIN_TILE;
    }
    bool ef, tf;
    S es, ts;
    win_block_exclusive(f, s, ef, es, tf, ts, lds_s, lds_f);
    if (j < ntiles) carry[j] = ef ? es : S::combine(run, es);
    run = tf ? ts : S::combine(run, ts);
  }
}

// C: fold the carry into the positions before the tile's first head; block b
// serves tile b + 1, tile 0 has nothing flowing in
template <class S, bool FWD>
__global__ __launch_bounds__(WIN_BLOCK) void win_apply_carry(
    S* __restrict__ out, const S* __restrict__ carry,
    const int* __restrict__ tile_first, int64_t n) {
  const int64_t tile = (int64_t)blockIdx.x + 1;
  const int first = tile_first[tile];
  const S c = carry[tile];
  for (int k = threadIdx.x; k < first; k += WIN_BLOCK) {
    int64_t q = tile * WIN_TILE + k;
    if (q < n) {
      int64_t p = win_pos<FWD>(q, n);
      out[p] = S::combine(c, out[p]);
    }
  }
}

// ---------------------------------------------------------------------------
// lookup
// ---------------------------------------------------------------------------
template <class S>
__global__ __launch_bounds__(WIN_BLOCK) void win_lookup(
    WinSeg sg, const S* __restrict__ F, const S* __restrict__ B,
    const PeerState* __restrict__ peer, int lo_kind, int64_t lo_off,
    int hi_kind, int64_t hi_off, int64_t w, int op,
    int64_t* __restrict__ value, int64_t* __restrict__ count) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < sg.n;
       p += stride) {
    int64_t row, ps, pe;
    win_bounds(sg, p, row, ps, pe);
    int64_t lo = lo_kind == WIN_UNBOUNDED ? ps : max(p + lo_off, ps);
    int64_t hi = pe;
    if (hi_kind == WIN_OFFSET) hi = min(p + hi_off, pe);
    else if (hi_kind == WIN_PEER_END) hi = max(p, min(peer[p].ext, pe));
    S r = S::identity();
    if (lo <= hi) {
      if (lo_kind == WIN_UNBOUNDED) {
        r = F[hi];
      } else if (hi_kind == WIN_UNBOUNDED) {
        r = B[lo];
      } else if (lo / w != hi / w) {
        r = S::combine(B[lo], F[hi]);  // disjoint: [lo, block end] + the rest
      } else {
        // same w-block: F[hi] starts at max(block start, ps); when that is
        // not lo, hi is the block end or pe and B[lo] ends there
        r = lo == max(lo / w * w, ps) ? F[hi] : B[lo];
      }
    }
    value[row] = r.cnt > 0 ? r.result_bits(op) : 0;
    count[row] = r.cnt;
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
namespace {

struct WinFrame {
  int lo_kind, hi_kind;
  int64_t lo_off, hi_off;
};

template <class S>
S* win_alloc(Tensor& keep, int64_t count, const torch::Device& dev) {
  keep = torch::empty({count * (int64_t)sizeof(S)},
                      torch::dtype(torch::kUInt8).device(dev));
  return reinterpret_cast<S*>(keep.data_ptr<uint8_t>());
}

// the three launches; `keep` holds the scan, the tile buffers die on return
// (stream-ordered, so the allocator reuses them only after the kernels)
template <class S, bool FWD, class Src>
S* win_scan(const Src& src, int64_t n, const torch::Device& dev,
            Tensor& keep) {
  const int64_t ntiles = (n + WIN_TILE - 1) / WIN_TILE;
  TORCH_CHECK(ntiles <= std::numeric_limits<int32_t>::max(),
              "window_agg: too many rows");
  Tensor t_state, t_carry;
  S* out = win_alloc<S>(keep, n, dev);
  S* tile_state = win_alloc<S>(t_state, ntiles, dev);
  S* carry = win_alloc<S>(t_carry, ntiles, dev);
  auto t_first = torch::empty({ntiles},
                              torch::dtype(torch::kInt32).device(dev));
  int* tile_first = t_first.data_ptr<int>();
  hipStream_t st = cur_stream();
  hipLaunchKernelGGL((win_scan_tiles<S, FWD, Src>), dim3((unsigned)ntiles),
                     dim3(WIN_BLOCK), 0, st, src, n, out, tile_state,
                     tile_first);
  if (ntiles > 1) {
    hipLaunchKernelGGL((win_scan_carries<S>), dim3(1), dim3(WIN_BLOCK), 0, st,
                       tile_state, tile_first, ntiles, carry);
    hipLaunchKernelGGL((win_apply_carry<S, FWD>), dim3((unsigned)(ntiles - 1)),
                       dim3(WIN_BLOCK), 0, st, out, carry, tile_first, n);
  }
  return out;
}

template <class S, class V>
void win_run(const WinSeg& sg, const V* values, const bool* valid,
             const bool* new_peer, const WinFrame& fr, int op,
             const torch::Device& dev, int64_t* value, int64_t* count) {
  const bool sliding = fr.lo_kind == WIN_OFFSET && fr.hi_kind == WIN_OFFSET;
  const int64_t w = sliding ? fr.hi_off - fr.lo_off + 1 : 0;
  Tensor keep_f, keep_b, keep_p;
  const S* F = nullptr;
  const S* B = nullptr;
  const PeerState* peer = nullptr;
  if (fr.lo_kind == WIN_UNBOUNDED || sliding)
    F = win_scan<S, true>(WinValueSrc<S, V, true>{sg, values, valid, w}, sg.n,
                          dev, keep_f);
  if (fr.lo_kind == WIN_OFFSET)
    B = win_scan<S, false>(WinValueSrc<S, V, false>{sg, values, valid, w},
                           sg.n, dev, keep_b);
  if (fr.hi_kind == WIN_PEER_END)
    peer = win_scan<PeerState, false>(WinPeerSrc{sg, new_peer}, sg.n, dev,
                                      keep_p);
  hipLaunchKernelGGL((win_lookup<S>), dim3(grid_1d(sg.n, WIN_BLOCK)),
                     dim3(WIN_BLOCK), 0, cur_stream(), sg, F, B, peer,
                     fr.lo_kind, fr.lo_off, fr.hi_kind, fr.hi_off, w, op,
                     value, count);
}

template <class V>
void win_dispatch(const WinSeg& sg, const V* values, const bool* valid,
                  const bool* new_peer, const WinFrame& fr, int op,
                  const torch::Device& dev, int64_t* value, int64_t* count) {
  switch (op) {
    case WIN_SUM:
    case WIN_MEAN:
      return win_run<SumState<V>, V>(sg, values, valid, new_peer, fr, op, dev,
                                     value, count);
    case WIN_MIN:
      return win_run<ExtState<V, false>, V>(sg, values, valid, new_peer, fr,
                                            op, dev, value, count);
    case WIN_MAX:
      return win_run<ExtState<V, true>, V>(sg, values, valid, new_peer, fr,
                                           op, dev, value, count);
    default:
      return win_run<VarState, V>(sg, values, valid, new_peer, fr, op, dev,
                                  value, count);
  }
}

}  // namespace

std::vector<Tensor> window_agg(OptTensor values, OptTensor valid, Tensor perm,
                               Tensor gids, Tensor seg_offsets,
                               OptTensor new_peer, int64_t lo_kind,
                               int64_t lo_off, int64_t hi_kind, int64_t hi_off,
                               int64_t op) {
  const char* who = "window_agg";
  TORCH_CHECK(perm.is_cuda(), who, ": perm must be on a GPU device");
  auto dev = perm.device();
  check_tensor(who, "perm", perm, torch::kInt64, dev);
  check_tensor(who, "gids", gids, torch::kInt64, dev);
  check_tensor(who, "seg_offsets", seg_offsets, torch::kInt64, dev);
  TORCH_CHECK(perm.dim() == 1 && gids.dim() == 1 && seg_offsets.dim() == 1,
              who, ": perm, gids and seg_offsets must be 1-D");
  const int64_t n = perm.numel();
  TORCH_CHECK(gids.numel() == n, who, ": gids must have ", n, " rows, got ",
              gids.numel());
  TORCH_CHECK(seg_offsets.numel() >= 2 || n == 0, who,
              ": seg_offsets must hold num_groups + 1 entries");
  TORCH_CHECK(op >= WIN_SUM && op <= WIN_STDDEV, who,
              ": op must be 0..6 (sum, count, mean, min, max, variance, "
              "stddev), got ", op);
  TORCH_CHECK(lo_kind == WIN_UNBOUNDED || lo_kind == WIN_OFFSET, who,
              ": lo_kind must be 0 (unbounded) or 1 (offset), got ", lo_kind);
  TORCH_CHECK(hi_kind >= WIN_UNBOUNDED && hi_kind <= WIN_PEER_END, who,
              ": hi_kind must be 0 (unbounded), 1 (offset) or 2 (peer end), "
              "got ", hi_kind);
  TORCH_CHECK(hi_kind != WIN_PEER_END || lo_kind == WIN_UNBOUNDED, who,
              ": a peer-end frame starts unbounded");
  bool is_float = false;
  if (op == WIN_COUNT) {
    values = c10::nullopt;  // a count reads validity only
  } else {
    TORCH_CHECK(values.has_value(), who, ": this op needs values");
    is_float = values->scalar_type() == torch::kFloat64;
    check_tensor(who, "values", *values,
                 is_float ? torch::kFloat64 : torch::kInt64, dev);
    TORCH_CHECK(values->dim() == 1 && values->numel() == n, who,
                ": values must be 1-D with ", n, " rows");
  }
  const bool* valid_p = check_valid(who, valid, n, dev);
  TORCH_CHECK(!valid.has_value() || valid->dim() == 1, who,
              ": valid must be 1-D");
  const bool* peer_p = nullptr;
  if (hi_kind == WIN_PEER_END) {
    TORCH_CHECK(new_peer.has_value(), who, ": a peer-end frame needs new_peer");
    check_tensor(who, "new_peer", *new_peer, torch::kBool, dev);
    TORCH_CHECK(new_peer->dim() == 1 && new_peer->numel() == n, who,
                ": new_peer must be 1-D with ", n, " rows");
    peer_p = new_peer->data_ptr<bool>();
  }

  const bool float_out = op == WIN_MEAN || op == WIN_VAR ||
                         op == WIN_STDDEV ||
                         (is_float && op != WIN_COUNT);
  auto i64 = torch::dtype(torch::kInt64).device(dev);
  const bool sliding = lo_kind == WIN_OFFSET && hi_kind == WIN_OFFSET;
  // n == 0, or a frame that is empty for every row: nothing to launch
  if (n == 0 || (sliding && lo_off > hi_off)) {
    auto value = torch::zeros({n}, i64);
    return {float_out ? value.view(torch::kFloat64) : value,
            torch::zeros({n}, i64)};
  }
  // an offset beyond +-n leaves every partition, as +-n does; the clamp keeps
  // p + offset and the frame width inside int64
  WinFrame fr{(int)lo_kind, (int)hi_kind,
              std::min(std::max(lo_off, -n), n),
              std::min(std::max(hi_off, -n), n)};
  WinSeg sg{perm.data_ptr<int64_t>(), gids.data_ptr<int64_t>(),
            seg_offsets.data_ptr<int64_t>(), n, seg_offsets.numel() - 1};
  auto value = torch::empty({n}, i64);
  auto count = torch::empty({n}, i64);
  int64_t* vp = value.data_ptr<int64_t>();
  int64_t* cp = count.data_ptr<int64_t>();
  if (op == WIN_COUNT)
    win_run<CntState, int64_t>(sg, nullptr, valid_p, peer_p, fr, (int)op, dev,
                               vp, cp);
  else if (is_float)
    win_dispatch<double>(sg, values->data_ptr<double>(), valid_p, peer_p, fr,
                         (int)op, dev, vp, cp);
  else
    win_dispatch<int64_t>(sg, values->data_ptr<int64_t>(), valid_p, peer_p,
                          fr, (int)op, dev, vp, cp);
  return {float_out ? value.view(torch::kFloat64) : value, count};
}
