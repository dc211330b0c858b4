// Structural CSV decode of one chunk in device memory (gfx950): which bytes
// separate fields and records once quotes are taken into account, and the
// selected columns cut out as Arrow offsets + bytes.
//
// A chunk is n < 2^31 bytes that begin at a record start.  Records end at
// '\n' (a '\r' before it belongs to the terminator), fields at `delim`; a
// field in '"' may hold either, and "" for one quote.  A byte is inside quotes
// exactly when the number of quotes before it is odd, so the whole structure
// follows from a prefix parity, and that parity is never carried serially
// along the bytes:
//
//   summary   one 256-thread block per 4096-byte tile, one 16-byte load per
//             thread.  Writes the tile's quote parity (ballot + 4 LDS words)
//             and the UTF-8 evidence: every lead byte checks its own
//             continuation bytes and the overlong, surrogate and > U+10FFFF
//             ranges of the first one, looking up to 3 bytes past the
//             thread's 16 (bounded global reads); the chunk-wide count of
//             continuation bytes claimed by leads minus those present must be
//             0.  A character cut off by the chunk's end is tolerated: a final
//             chunk ends in '\n', any other keeps that tail for the next.
//   (host)    exclusive xor scan of the n/4096 tile parities: torch.cumsum.
//   classify  same tiling.  16-bit masks of quote, delim, '\n', '\r' per
//             thread; in-thread prefix xor by shifts; the lane's incoming
//             parity is one ballot of the lanes' parities masked to lower
//             lanes; waves combine through 4 LDS words and the tile's scanned
//             parity.  Stores the 16-bit mask of separators outside quotes
//             (2 B per 16 B of input) and the tile's separator count, and
//             checks that every quote is regular: met at even parity it
//             follows a separator, the chunk start or a quote; met at odd
//             parity a separator, "\r\n", the chunk end or a quote follows.
//             A '\r' outside quotes that no '\n' follows is flagged too:
//             pyarrow ends a record there, these kernels do not.
//             Neighbours across thread and tile borders are bounded global
//             reads, made only by threads that have a quote or a '\r' at
//             their border.
//   (host)    exclusive scan of the tile counts: torch.cumsum.
//   emit      one block per tile reads the stored masks and writes sep_pos
//             int32 [S] in byte order: tile base + wave base (block_rank.h)
//             + lane base, the last a wave prefix sum of popcounts since a
//             lane holds up to 16 separators.
//   rowcheck  one thread per separator: it must be a '\n' exactly when
//             (s + 1) % ncols == 0 (else ragged); an empty record sets
//             blank_line; a wave-reduced atomicMax gives the last '\n'
//             separator (consumed).
//   lens      one thread per field (row r, selected column c) between
//             sep_pos[r * ncols + c - 1] + 1 and sep_pos[r * ncols + c].  An
//             unquoted field's length is the difference of two positions; it
//             is never read byte by byte.  A field that starts with '"' loses
//             the outer quotes and half of the quotes inside, which are
//             counted by its thread, or, past kLongField bytes, by the whole
//             wave: the ballot of such lanes is walked, the span broadcast by
//             shuffle, the 64 lanes stride over it and reduce.
//   extract   a column without quoted fields is one launch_copy_segments;
//             otherwise the unescape kernel writes it, long fields again by
//             the wave: 64 bytes per step, a byte's output slot is its index
//             minus half the quotes before it (ballot rank plus the carried
//             count), and the second quote of each pair is dropped.
//
// All flags and counts come back in one int32 [8] tensor (kInfo*).  Columns
// that are not selected are never touched.
#include "common.h"
#include "block_rank.h"
#include "bytes16.h"
#include "host_args.h"
#include "api.h"

#include <climits>

constexpr int kCsvBlock = 256;
constexpr int kCsvTile = kCsvBlock * 16;
constexpr int kCsvWaves = kCsvBlock / WAVE;
constexpr int kLongField = 256;  // bytes from which a wave shares a field

enum : int32_t {
  kIrregular = 1, kBadUtf8 = 2, kRagged = 4, kBlankLine = 8, kBareCr = 16
};
enum {
  kInfoErr = 0,        // the bits above
  kInfoCont = 1,       // continuation bytes claimed - present
  kInfoConsumed = 2,   // position of the last '\n' separator + 1
  kInfoSeps = 3,       // S
  kInfoEndParity = 4,  // 1: the chunk ends inside quotes
  kInfoLen = 8
};

// ---------------------------------------------------------------------------
// summary: quote parity and UTF-8 evidence of a tile
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kCsvBlock)
csv_summary_kernel(const uint8_t* data, int64_t n, int32_t* tile_parity,
                   int32_t* info) {
  __shared__ int32_t wpar[kCsvWaves];
  const int64_t base = (int64_t)blockIdx.x * kCsvTile + threadIdx.x * 16;
  Bytes16 b{0, 0};
  if (base < n) b = load16(data, n, base);
  int diff = 0;
  bool bad = utf8_evidence(data, n, base, b, &diff);
  if (bad) atomicOr(info + kInfoErr, kBadUtf8);
  int32_t total = block_sum(diff);
  if (threadIdx.x == 0 && total) atomicAdd(info + kInfoCont, total);

  uint64_t odd = __ballot(__popc(eq_mask(b, '"')) & 1);
  wave_total_put(wpar, __popcll(odd) & 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t p = 0;
    for (int w = 0; w < kCsvWaves; ++w) p ^= wpar[w];
    tile_parity[blockIdx.x] = p;
  }
}

// ---------------------------------------------------------------------------
// classify: separators outside quotes, regular quotes
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kCsvBlock)
csv_classify_kernel(const uint8_t* data, int64_t n, uint32_t delim,
                    const int32_t* tile_parity_in, uint16_t* sepmask,
                    int32_t* tile_count, int32_t* info) {
  __shared__ int32_t wpar[kCsvWaves];
  const int64_t base = (int64_t)blockIdx.x * kCsvTile + threadIdx.x * 16;
  Bytes16 b{0, 0};
  if (base < n) b = load16(data, n, base);
  const uint32_t q = eq_mask(b, '"'), d = eq_mask(b, delim);
  const uint32_t nl = eq_mask(b, '\n'), cr = eq_mask(b, '\r');
  uint32_t x = q;  // bit i: parity of the thread's quotes in bytes [0, i]
  x ^= x << 1;
  x ^= x << 2;
  x ^= x << 4;
  x ^= x << 8;
  x &= 0xFFFF;
  uint64_t odd = __ballot((x >> 15) & 1);
  wave_total_put(wpar, __popcll(odd) & 1);
  __syncthreads();
  uint32_t in = tile_parity_in[blockIdx.x] ^
                (__popcll(odd & lane_lt_mask()) & 1);
  for (int w = 0; w < wave_id(); ++w) in ^= wpar[w];
  const uint32_t incl = x ^ (in ? 0xFFFFu : 0u);          // after byte i
  const uint32_t before = ((incl << 1) | in) & 0xFFFF;    // before byte i
  const uint32_t sep = (d | nl) & ~incl & 0xFFFF;

  // quotes met outside quotes: the byte before is a separator or a quote
  const uint32_t opens = q & ~before;
  uint32_t prev_ok = ((d | nl | q) << 1) & 0xFFFF;
  if (opens & 1) {
    uint32_t pb = base > 0 ? data[base - 1] : delim;
    prev_ok |= pb == '"' || pb == delim || pb == '\n';
  }
  // quotes met inside quotes: a separator, "\r\n", the end or a quote follows
  const uint32_t closes = q & before;
  const uint32_t cr_out = cr & ~incl & 0xFFFF;   // '\r' outside quotes
  uint32_t ok = q | d | nl, crs = cr, nls = nl;  // 18 bits: bytes 0 .. 17
  if ((closes & 0xC000) | (cr_out & 0x8000)) {
    for (int j = 16; j < 18; ++j) {
      if (base + j >= n) break;
      uint32_t c = data[base + j];
      ok |= (uint32_t)(c == '"' || c == delim || c == '\n') << j;
      crs |= (uint32_t)(c == '\r') << j;
      nls |= (uint32_t)(c == '\n') << j;
    }
  }
  int64_t left = n - base;  // bytes of the chunk from `base` on
  uint32_t endm = left >= 18 ? 0u : left <= 0 ? 0x3FFFFu
                                              : (0x3FFFFu << left) & 0x3FFFFu;
  ok |= endm | (crs & ((nls | endm) >> 1));
  if ((opens & ~prev_ok) | (closes & ~(ok >> 1)))
    atomicOr(info + kInfoErr, kIrregular);
  // a '\r' at the chunk's end may still get its '\n' from the next block
  if (cr_out & ~((nls | endm) >> 1)) atomicOr(info + kInfoErr, kBareCr);

  sepmask[(int64_t)blockIdx.x * kCsvBlock + threadIdx.x] = (uint16_t)sep;
  int32_t total = block_sum(__popc(sep));
  if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------
// emit: separator positions in byte order
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kCsvBlock)
csv_emit_kernel(const uint16_t* sepmask, const int32_t* tile_base, int64_t S,
                int32_t* sep_pos) {
  __shared__ int32_t row[kCsvWaves];
  uint32_t m = sepmask[(int64_t)blockIdx.x * kCsvBlock + threadIdx.x];
  const int c = __popc(m);
  int v = c;  // inclusive prefix sum over the wave
  for (int off = 1; off < WAVE; off <<= 1) {
    int t = __shfl_up(v, off, WAVE);
    if (lane_id() >= off) v += t;
  }
  wave_total_put(row, __shfl(v, WAVE - 1, WAVE));
  __syncthreads();
  WaveSpan span = wave_span<kCsvWaves>(row);
  int64_t o = (int64_t)tile_base[blockIdx.x] + span.before + (v - c);
  const int64_t pos0 = (int64_t)blockIdx.x * kCsvTile + threadIdx.x * 16;
  for (; m; m &= m - 1, ++o)
    if (o < S) sep_pos[o] = (int32_t)(pos0 + __ffs(m) - 1);
}

// ---------------------------------------------------------------------------
// rowcheck: every ncols-th separator ends a record, and no other
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kCsvBlock)
csv_rowcheck_kernel(const uint8_t* data, const int32_t* sep_pos, int64_t S,
                    int64_t ncols, int32_t* info) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t s0 = (int64_t)blockIdx.x * blockDim.x; s0 < S; s0 += stride) {
    const int64_t s = s0 + threadIdx.x;
    int32_t end1 = 0, err = 0;
    if (s < S) {
      int32_t p = sep_pos[s];
      bool is_nl = data[p] == '\n';
      if (is_nl != ((s + 1) % ncols == 0)) err |= kRagged;
      if (is_nl) {
        end1 = p + 1;
        int32_t prev = s ? sep_pos[s - 1] : -1;
        bool at_start = s == 0 || data[prev] == '\n';
        if (at_start &&
            (p == prev + 1 || (p == prev + 2 && data[prev + 1] == '\r')))
          err |= kBlankLine;
      }
    }
    for (int off = WAVE / 2; off; off >>= 1) {
      end1 = max(end1, __shfl_xor(end1, off, WAVE));
      err |= __shfl_xor(err, off, WAVE);
    }
    if (lane_id() == 0) {
      if (end1) atomicMax(info + kInfoConsumed, end1);
      if (err) atomicOr(info + kInfoErr, err);
    }
  }
}

// ---------------------------------------------------------------------------
// fields
// ---------------------------------------------------------------------------
// content of field `idx`: [*a, *e), outer quotes and the terminator's '\r'
// left out
DEV_INLINE bool field_span(const uint8_t* data, const int32_t* sep_pos,
                           int64_t idx, bool last_col, int32_t* a,
                           int32_t* e) {
  int32_t s = idx ? sep_pos[idx - 1] + 1 : 0, t = sep_pos[idx];
  if (last_col && t > s && data[t - 1] == '\r') --t;
  bool quoted = t - s >= 2 && data[s] == '"';
  *a = quoted ? s + 1 : s;
  *e = quoted ? t - 1 : t;
  return quoted;
}

// blockIdx.y is the selected column, the x dimension strides over rows
__global__ void __launch_bounds__(kCsvBlock)
csv_lens_kernel(const uint8_t* data, const int32_t* sep_pos, int64_t ncols,
                int64_t row0, int64_t nrows, const int32_t* cols,
                int64_t* seg_start, int64_t* lens, int32_t* any_quoted) {
  const int j = blockIdx.y;
  const int64_t c = cols[j];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r0 = (int64_t)blockIdx.x * blockDim.x; r0 < nrows;
       r0 += stride) {
    const int64_t r = r0 + threadIdx.x;
    int32_t a = 0, e = 0;
    bool quoted = false;
    if (r < nrows)
      quoted = field_span(data, sep_pos, (row0 + r) * ncols + c,
                          c == ncols - 1, &a, &e);
    int quotes = 0;
    bool is_long = quoted && e - a > kLongField;
    if (quoted && !is_long)
      for (int32_t p = a; p < e; ++p) quotes += data[p] == '"';
    for (uint64_t todo = __ballot(is_long); todo; todo &= todo - 1) {
      int src = __ffsll((unsigned long long)todo) - 1;
      int32_t sa = __shfl(a, src, WAVE), se = __shfl(e, src, WAVE);
      int cnt = 0;
      for (int32_t p = sa + lane_id(); p < se; p += WAVE)
        cnt += data[p] == '"';
      cnt = wave_sum(cnt);
      if (lane_id() == src) quotes = cnt;
    }
    if (r < nrows) {
      seg_start[j * nrows + r] = a;
      lens[j * nrows + r] = (e - a) - quotes / 2;
    }
    if (__ballot(quoted) && lane_id() == 0) atomicOr(any_quoted + j, 1);
  }
}

// one column with quoted fields: copy, dropping the second quote of each ""
__global__ void __launch_bounds__(kCsvBlock)
csv_unescape_kernel(const uint8_t* data, const int32_t* sep_pos, int64_t ncols,
                    int64_t row0, int64_t nrows, int64_t c,
                    const int64_t* out_offs, int64_t total, uint8_t* out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r0 = (int64_t)blockIdx.x * blockDim.x; r0 < nrows;
       r0 += stride) {
    const int64_t r = r0 + threadIdx.x;
    int32_t a = 0, e = 0;
    int64_t o = 0;
    if (r < nrows) {
      field_span(data, sep_pos, (row0 + r) * ncols + c, c == ncols - 1, &a,
                 &e);
      o = out_offs[r];
    }
    bool is_long = e - a > kLongField;
    if (!is_long) {
      int quotes = 0;  // met so far; an odd count drops the next one
      for (int32_t p = a; p < e; ++p) {
        uint8_t ch = data[p];
        if (ch == '"' && (quotes++ & 1)) continue;
        if (o >= 0 && o < total) out[o] = ch;
        ++o;
      }
    }
    for (uint64_t todo = __ballot(is_long); todo; todo &= todo - 1) {
      int src = __ffsll((unsigned long long)todo) - 1;
      int32_t sa = __shfl(a, src, WAVE), se = __shfl(e, src, WAVE);
      int64_t so = __shfl(o, src, WAVE);
      int carried = 0;
      for (int32_t p0 = sa; p0 < se; p0 += WAVE) {
        int32_t p = p0 + lane_id();
        uint8_t ch = p < se ? data[p] : 0;
        bool is_q = p < se && ch == '"';
        uint64_t qs = __ballot(is_q);
        int before = carried + __popcll(qs & lane_lt_mask());
        int64_t at = so + (p - sa) - before / 2;
        if (p < se && !(is_q && (before & 1)) && at >= 0 && at < total)
          out[at] = ch;
        carried += __popcll(qs);
      }
    }
  }
}

// Rows that str_parse_* answers with status 0 where pyarrow's CSV converters
// answer otherwise become status 2.  kind 0: signed integer, a leading '+';
// kind 1: unsigned integer, a leading '+' or '-'; kind 2: decimal, more
// fractional digits than `scale`.
__global__ void csv_precheck_kernel(const int64_t* offs, const uint8_t* bytes,
                                    int64_t nbytes, int64_t n, int kind,
                                    int scale, uint8_t* status) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n;
       r += stride) {
    int64_t a = offs[r], e = offs[r + 1];
    if (status[r] != 0 || a < 0 || a >= e || e > nbytes) continue;
    uint8_t c0 = bytes[a];
    bool host = false;
    if (kind == 0) host = c0 == '+';
    if (kind == 1) host = c0 == '+' || c0 == '-';
    if (kind == 2) {
      int64_t dot = a;
      while (dot < e && bytes[dot] != '.') ++dot;
      host = e - dot - 1 > scale;
    }
    if (host) status[r] = 2;
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
static int64_t check_chunk(const char* who, const Tensor& data) {
  TORCH_CHECK(data.is_cuda(), who, ": data must be on a GPU device");
  check_tensor(who, "data", data, torch::kUInt8, data.device());
  TORCH_CHECK(data.dim() == 1 && data.numel() < (int64_t)INT_MAX, who,
              ": data must be one chunk of fewer than 2^31 bytes");
  TORCH_CHECK(data.numel() == 0 || (uintptr_t)data.data_ptr() % 16 == 0, who,
              ": data must be 16-byte aligned");
  return data.numel();
}

static const int32_t* check_seps(const char* who, const Tensor& sep_pos,
                                 const Tensor& data, int64_t ncols,
                                 int64_t row0, int64_t nrows) {
  check_tensor(who, "sep_pos", sep_pos, torch::kInt32, data.device());
  TORCH_CHECK(ncols >= 1 && row0 >= 0 && nrows >= 0 &&
                  (row0 + nrows) * ncols <= sep_pos.numel(),
              who, ": rows [", row0, ", ", row0 + nrows, ") of ", ncols,
              " columns need more separators than the ", sep_pos.numel(),
              " given");
  return sep_pos.numel() ? sep_pos.data_ptr<int32_t>() : nullptr;
}

std::vector<Tensor> csv_structure(Tensor data, int64_t delim) {
  const int64_t n = check_chunk("csv_structure", data);
  TORCH_CHECK(delim > 0 && delim < 128 && delim != '"' && delim != '\n' &&
                  delim != '\r',
              "csv_structure: delim must be one ASCII byte other than "
              "'\"', '\\n' and '\\r', got ", delim);
  auto dev = data.device();
  auto i32 = torch::dtype(torch::kInt32).device(dev);
  const int64_t ntiles = (n + kCsvTile - 1) / kCsvTile;
  auto info = torch::zeros({kInfoLen}, i32);
  auto sepmask = torch::empty({ntiles * kCsvBlock},
                              torch::dtype(torch::kInt16).device(dev));
  if (n == 0) return {sepmask, torch::empty({0}, i32), info};
  auto parity = torch::empty({ntiles}, i32);
  auto counts = torch::empty({ntiles}, i32);
  hipLaunchKernelGGL(csv_summary_kernel, dim3((unsigned)ntiles),
                     dim3(kCsvBlock), 0, cur_stream(), data.data_ptr<uint8_t>(),
                     n, parity.data_ptr<int32_t>(), info.data_ptr<int32_t>());
  auto incl = torch::cumsum(parity, 0);
  auto parity_in = ((incl - parity) & 1).to(torch::kInt32);
  info.select(0, kInfoEndParity).copy_(incl[ntiles - 1] & 1);
  hipLaunchKernelGGL(csv_classify_kernel, dim3((unsigned)ntiles),
                     dim3(kCsvBlock), 0, cur_stream(), data.data_ptr<uint8_t>(),
                     n, (uint32_t)delim, parity_in.data_ptr<int32_t>(),
                     (uint16_t*)sepmask.data_ptr<int16_t>(),
                     counts.data_ptr<int32_t>(), info.data_ptr<int32_t>());
  auto run = torch::cumsum(counts, 0);
  info.select(0, kInfoSeps).copy_(run[ntiles - 1]);
  return {sepmask, (run - counts).to(torch::kInt32), info};
}

Tensor csv_emit(Tensor data, Tensor sepmask, Tensor tile_base, Tensor info,
                int64_t S, int64_t ncols) {
  const int64_t n = check_chunk("csv_emit", data);
  auto dev = data.device();
  const int64_t ntiles = (n + kCsvTile - 1) / kCsvTile;
  check_tensor("csv_emit", "sepmask", sepmask, torch::kInt16, dev);
  check_tensor("csv_emit", "tile_base", tile_base, torch::kInt32, dev);
  check_tensor("csv_emit", "info", info, torch::kInt32, dev);
  TORCH_CHECK(sepmask.numel() == ntiles * kCsvBlock &&
                  tile_base.numel() == ntiles && info.numel() == kInfoLen,
              "csv_emit: sepmask, tile_base and info must be csv_structure's "
              "for this chunk");
  TORCH_CHECK(S >= 0 && S <= n && ncols >= 1,
              "csv_emit: need 0 <= S <= n and ncols >= 1, got S ", S,
              ", ncols ", ncols);
  auto sep_pos = torch::empty({S}, torch::dtype(torch::kInt32).device(dev));
  if (S == 0) return sep_pos;
  hipLaunchKernelGGL(csv_emit_kernel, dim3((unsigned)ntiles), dim3(kCsvBlock),
                     0, cur_stream(),
                     (const uint16_t*)sepmask.data_ptr<int16_t>(),
                     tile_base.data_ptr<int32_t>(), S,
                     sep_pos.data_ptr<int32_t>());
  hipLaunchKernelGGL(csv_rowcheck_kernel, dim3(grid_1d(S, kCsvBlock)),
                     dim3(kCsvBlock), 0, cur_stream(), data.data_ptr<uint8_t>(),
                     sep_pos.data_ptr<int32_t>(), S, ncols,
                     info.data_ptr<int32_t>());
  return sep_pos;
}

std::vector<Tensor> csv_field_lens(Tensor data, Tensor sep_pos, int64_t ncols,
                                   int64_t row0, int64_t nrows,
                                   std::vector<int64_t> cols) {
  check_chunk("csv_field_lens", data);
  const int32_t* seps =
      check_seps("csv_field_lens", sep_pos, data, ncols, row0, nrows);
  const int64_t nsel = (int64_t)cols.size();
  TORCH_CHECK(nsel <= 65535, "csv_field_lens: at most 65535 columns");
  for (int64_t c : cols)
    TORCH_CHECK(c >= 0 && c < ncols, "csv_field_lens: column ", c,
                " is not in [0, ", ncols, ")");
  auto dev = data.device();
  auto i64 = torch::dtype(torch::kInt64).device(dev);
  auto seg_start = torch::empty({nsel, nrows}, i64);
  auto lens = torch::empty({nsel, nrows}, i64);
  auto any_quoted =
      torch::zeros({nsel}, torch::dtype(torch::kInt32).device(dev));
  if (nsel == 0 || nrows == 0) return {seg_start, lens, any_quoted};
  auto cols_dev = torch::tensor(at::ArrayRef<int64_t>(cols),
                                torch::dtype(torch::kInt32)).to(dev);
  int gx = std::min(grid_1d(nrows, kCsvBlock), 1024);
  hipLaunchKernelGGL(csv_lens_kernel, dim3(gx, (unsigned)nsel),
                     dim3(kCsvBlock), 0, cur_stream(), data.data_ptr<uint8_t>(),
                     seps, ncols, row0, nrows, cols_dev.data_ptr<int32_t>(),
                     seg_start.data_ptr<int64_t>(), lens.data_ptr<int64_t>(),
                     any_quoted.data_ptr<int32_t>());
  return {seg_start, lens, any_quoted};
}

Tensor csv_extract(Tensor data, Tensor sep_pos, int64_t ncols, int64_t row0,
                   int64_t col, Tensor seg_start, Tensor out_offsets,
                   int64_t total, bool quoted) {
  const int64_t n = check_chunk("csv_extract", data);
  auto dev = data.device();
  check_tensor("csv_extract", "out_offsets", out_offsets, torch::kInt64, dev);
  check_tensor("csv_extract", "seg_start", seg_start, torch::kInt64, dev);
  TORCH_CHECK(out_offsets.dim() == 1 && out_offsets.numel() >= 1 &&
                  seg_start.numel() == out_offsets.numel() - 1,
              "csv_extract: out_offsets must be [nrows + 1] and seg_start "
              "[nrows]");
  const int64_t nrows = seg_start.numel();
  const int32_t* seps =
      check_seps("csv_extract", sep_pos, data, ncols, row0, nrows);
  TORCH_CHECK(col >= 0 && col < ncols && total >= 0 && total <= n,
              "csv_extract: need 0 <= col < ncols and 0 <= total <= n");
  auto out = torch::empty({total}, torch::dtype(torch::kUInt8).device(dev));
  if (total == 0 || nrows == 0) return out;
  if (!quoted) {
    launch_copy_segments(data.data_ptr<uint8_t>(), n,
                         seg_start.data_ptr<int64_t>(),
                         out_offsets.data_ptr<int64_t>(), nrows, total,
                         out.data_ptr<uint8_t>());
  } else {
    hipLaunchKernelGGL(csv_unescape_kernel, dim3(grid_1d(nrows, kCsvBlock)),
                       dim3(kCsvBlock), 0, cur_stream(),
                       data.data_ptr<uint8_t>(), seps, ncols, row0, nrows, col,
                       out_offsets.data_ptr<int64_t>(), total,
                       out.data_ptr<uint8_t>());
  }
  return out;
}

void csv_precheck(Tensor offsets, Tensor bytes, Tensor status, int64_t kind,
                  int64_t scale) {
  StrCol c = check_strcol("csv_precheck", offsets, bytes);
  check_tensor("csv_precheck", "status", status, torch::kUInt8,
               offsets.device());
  TORCH_CHECK(status.numel() == c.n && kind >= 0 && kind <= 2 && scale >= 0,
              "csv_precheck: status must have one entry per row, kind in "
              "[0, 2], scale >= 0");
  if (c.n == 0) return;
  hipLaunchKernelGGL(csv_precheck_kernel, dim3(grid_1d(c.n, 256)), dim3(256),
                     0, cur_stream(), c.offs, c.bytes, c.nbytes, c.n,
                     (int)kind, (int)std::min<int64_t>(scale, 1 << 20),
                     status.data_ptr<uint8_t>());
}
