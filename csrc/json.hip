// Structural JSON-lines decode of one chunk in device memory (gfx950): which
// bytes are inside strings once backslash escapes are taken into account,
// the nesting depth of every structural byte, the fields of every record
// found by key, and the values of the schema's columns cut out (strings
// unescaped) as Arrow offsets + bytes.
//
// A chunk is n < 2^31 bytes that begin at a record start.  A record is one
// object; records are separated by whitespace, and a '\n' at depth 0 ends a
// line.  The tiling is csv.hip's: 256-thread blocks, one 16-byte load per
// thread, 4096-byte tiles, tile carries scanned by torch.cumsum between
// launches, all flags and counts in one int32 [8] tensor (kJ*).
//
//   summary   a byte is escaped when an odd run of '\' precedes it: inside a
//             thread's 16 bytes by mask arithmetic (one add carries every
//             run), a run that reaches the thread's first byte by a backward
//             read of at most kMaxBackslashRun bytes (longer: long_escape_run).
//             Real quotes are '"' bytes that are not escaped; the tile's
//             parity of them goes through a ballot and 4 LDS words.  UTF-8
//             evidence as in csv.hip (bytes16.h).
//   classify  with the scanned parity: bytes inside strings, the structural
//             bytes { } [ ] : , '\n' outside them (stored as a 16-bit mask),
//             the tile's depth delta.  Flags any other byte outside strings
//             that is neither whitespace nor a scalar's character, and a raw
//             byte below 0x20 inside a string.
//   tokens    with the scanned depth, twice: a counting pass (tokens and
//             record ends per tile, `consumed` = one past the last '\n' at
//             depth 0, depth errors), and after their scans a writing pass.
//             A token is a depth-0->1 '{', a depth-1 ':' or ',', or the
//             depth-1->0 '}'; it holds its position, its kind and its row:
//             the number of record-closing '}' before it.  Slots come from
//             tile base + wave base (block_rank.h) + lane base.
//   fields    one thread per token: neighbour kinds ('{' -> ':' or '}',
//             ':' -> ',' or '}', ',' -> ':'), whitespace between records,
//             and for a ':' the key before it, looked up in the schema's
//             names, which are staged in LDS as a hash table, offsets and
//             bytes.  field_tok[col, row] gets the token by atomicCAS, which
//             also finds a key that is met twice.
//   values    one thread per (column, row): the trimmed span between the ':'
//             and the next token is null, false, true, a number (checked
//             against the JSON grammar), a string (its unescaped length, its
//             escapes checked) or nested text.  Strings of kLongValue bytes
//             or more are walked by the whole wave, 64 bytes per step.
//   extract   string content without any backslash is launch_copy_segments;
//             otherwise the unescape kernel writes it, long values again by
//             the wave: a byte's slot is its index minus the bytes dropped
//             before it, the dropped count is carried across steps, and an
//             escape cut by a step boundary belongs to the step it starts in.
#include "common.h"
#include "block_rank.h"
#include "bytes16.h"
#include "host_args.h"
#include "api.h"

#include <climits>
#include <string>

constexpr int kJBlock = 256;
constexpr int kJTile = kJBlock * 16;
constexpr int kJWaves = kJBlock / WAVE;
constexpr int kLongValue = 256;        // bytes from which a wave shares a string
constexpr int kMaxBackslashRun = 64;   // backward read of a run of '\'
constexpr int kMaxKeys = 256;          // schema names staged in LDS
constexpr int kMaxKeyBytes = 2048;
constexpr int kKeyHash = 512;          // slots, load factor <= 0.5
constexpr int kKeyWords = 2 + kKeyHash + (kMaxKeys + 1) + kMaxKeyBytes / 4;

enum : int32_t {
  kJIrregular = 1, kJBadUtf8 = 2, kJLongRun = 4, kJDepth = 8, kJKeyEscape = 16,
  kJUnknownKey = 32, kJDupKey = 64, kJBadEscape = 128, kJControl = 256
};
enum {
  kJErr = 0,        // the bits above
  kJCont = 1,       // continuation bytes claimed - present
  kJConsumed = 2,   // one past the last '\n' at depth 0
  kJTokens = 3,     // T
  kJEndParity = 4,  // 1: the chunk ends inside a string
  kJMaxRecord = 5,  // bytes of the longest record
  kJRows = 6,       // records that end before `consumed`
  kJCloses = 7,     // record-closing '}' in the whole chunk
  kJInfoLen = 8
};
enum { kNull = 0, kFalse = 1, kTrue = 2, kNumber = 3, kString = 4, kNested = 5 };

// ---------------------------------------------------------------------------
// escapes and quotes of a thread's 16 bytes
// ---------------------------------------------------------------------------
// bit i: byte i is escaped.  bs: the '\' bytes; prev: the first byte is
// escaped.  Runs that start on an odd bit are added to the mask, so the carry
// of the add lands behind every run and tells its length's parity.
DEV_INLINE uint32_t escaped_mask(uint32_t bs, uint32_t prev) {
  bs &= ~prev;
  const uint32_t follows = (bs << 1) | prev, even = 0x5555u;
  const uint32_t odd_starts = bs & ~even & ~follows;
  const uint32_t invert = (odd_starts + bs) << 1;
  return (even ^ invert) & follows & 0xFFFF;
}

DEV_INLINE uint32_t real_quotes(const uint8_t* data, int64_t base,
                                const Bytes16& b, bool* long_run) {
  const uint32_t q = eq_mask(b, '"'), bs = eq_mask(b, '\\');
  uint32_t prev = 0;
  if (((q | bs) & 1) && base > 0) {  // else the first byte's state is unused
    int k = 0;
    while (k < kMaxBackslashRun && base - 1 - k >= 0 &&
           data[base - 1 - k] == '\\')
      ++k;
    if (k == kMaxBackslashRun) *long_run = true;
    prev = k & 1;
  }
  return q & ~escaped_mask(bs, prev);
}

// exclusive prefix of v over the block's threads; *total is the block's sum.
// One barrier; `row` is an LDS row of kJWaves cells used by nothing else.
DEV_INLINE int block_excl(int v, int32_t* row, int* total) {
  int s = v;
  for (int off = 1; off < WAVE; off <<= 1) {
    int t = __shfl_up(s, off, WAVE);
    if (lane_id() >= off) s += t;
  }
  wave_total_put(row, __shfl(s, WAVE - 1, WAVE));
  __syncthreads();
  WaveSpan span = wave_span<kJWaves>(row);
  *total = span.total;
  return span.before + s - v;
}

// ---------------------------------------------------------------------------
// summary: real-quote parity and UTF-8 evidence of a tile
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kJBlock)
json_summary_kernel(const uint8_t* data, int64_t n, int32_t* tile_parity,
                    int32_t* info) {
  __shared__ int32_t wpar[kJWaves];
  const int64_t base = (int64_t)blockIdx.x * kJTile + threadIdx.x * 16;
  Bytes16 b{0, 0};
  if (base < n) b = load16(data, n, base);
  int diff = 0;
  if (utf8_evidence(data, n, base, b, &diff)) atomicOr(info + kJErr, kJBadUtf8);
  int32_t total = block_sum(diff);
  if (threadIdx.x == 0 && total) atomicAdd(info + kJCont, total);

  bool long_run = false;
  const uint32_t rq = real_quotes(data, base, b, &long_run);
  if (long_run) atomicOr(info + kJErr, kJLongRun);
  uint64_t odd = __ballot(__popc(rq) & 1);
  wave_total_put(wpar, __popcll(odd) & 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t p = 0;
    for (int w = 0; w < kJWaves; ++w) p ^= wpar[w];
    tile_parity[blockIdx.x] = p;
  }
}

// ---------------------------------------------------------------------------
// classify: structural bytes outside strings, the tile's depth delta
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kJBlock)
json_classify_kernel(const uint8_t* data, int64_t n,
                     const int32_t* tile_parity_in, uint16_t* structmask,
                     int32_t* tile_depth, int32_t* info) {
  __shared__ int32_t wpar[kJWaves];
  const int64_t base = (int64_t)blockIdx.x * kJTile + threadIdx.x * 16;
  Bytes16 b{0, 0};
  if (base < n) b = load16(data, n, base);
  bool long_run = false;
  uint32_t x = real_quotes(data, base, b, &long_run);
  x ^= x << 1;  // bit i: parity of the thread's real quotes in bytes [0, i]
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
  const uint32_t incl = x ^ (in ? 0xFFFFu : 0u);        // after byte i
  const uint32_t before = ((incl << 1) | in) & 0xFFFF;  // before byte i
  const int64_t left = n - base;
  const uint32_t live = left >= 16 ? 0xFFFFu : left <= 0 ? 0u : (1u << left) - 1;
  const uint32_t content = before & incl & live;  // between a string's quotes
  const uint32_t outside = ~(before | incl) & live;

  uint32_t open = 0, close = 0, other = 0, space = 0, scalar = 0, low = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t c = byte_of(b, i), bit = 1u << i;
    if (c == '{' || c == '[') open |= bit;
    if (c == '}' || c == ']') close |= bit;
    if (c == ':' || c == ',' || c == '\n') other |= bit;
    if (c == ' ' || c == '\t' || c == '\r' || c == '\n') space |= bit;
    if ((c >= '0' && c <= '9') || ((c | 0x20) >= 'a' && (c | 0x20) <= 'z') ||
        c == '+' || c == '-' || c == '.')
      scalar |= bit;
    if (c < 0x20) low |= bit;
  }
  const uint32_t structural = (open | close | other) & outside;
  int32_t err = 0;
  if (outside & ~(structural | space | scalar)) err |= kJIrregular;
  if (content & low) err |= kJControl;
  if (err) atomicOr(info + kJErr, err);

  structmask[(int64_t)blockIdx.x * kJBlock + threadIdx.x] =
      (uint16_t)structural;
  int32_t total = block_sum(__popc(open & outside) - __popc(close & outside));
  if (threadIdx.x == 0) tile_depth[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------
// tokens: the depth-1 structure in byte order
// ---------------------------------------------------------------------------
// Walks the thread's structural bytes from depth d.  Returns its tokens;
// with kWrite they go to slots o, o + 1, ... and rows count on from `row`.
template <bool kWrite>
DEV_INLINE int walk_tokens(const Bytes16& b, uint32_t m, int d, int64_t pos0,
                           int64_t o, uint32_t row, int64_t T,
                           int32_t* tok_pos, int32_t* tok_meta, int* ncloses,
                           int32_t* err, int32_t* consumed) {
  int ntok = 0;
  for (; m; m &= m - 1) {
    const int i = __ffs(m) - 1;
    const uint32_t c = byte_of(b, i);
    int kind = -1;
    if (c == '{') {
      if (d == 0) kind = 0;
      ++d;
    } else if (c == '[') {
      if (d == 0) *err |= kJIrregular;  // a top-level array is not a record
      ++d;
    } else if (c == '}') {
      --d;
      if (d == 0) kind = 3;
      if (d < 0) *err |= kJDepth;
    } else if (c == ']') {
      --d;
      if (d <= 0) *err |= kJDepth;
    } else if (c == '\n') {
      if (d == 0) *consumed = (int32_t)(pos0 + i + 1);
      else *err |= kJDepth;  // a line ends inside a record
    } else {
      if (d == 1) kind = c == ':' ? 1 : 2;
      if (d <= 0) *err |= kJIrregular;
    }
    if (kind < 0) continue;
    if (kWrite && o + ntok < T) {
      tok_pos[o + ntok] = (int32_t)(pos0 + i);
      tok_meta[o + ntok] = (int32_t)((row << 2) | (uint32_t)kind);
    }
    ++ntok;
    if (kind == 3) {
      ++*ncloses;
      ++row;
    }
  }
  return ntok;
}

// kWrite false: tile_counts[tile] = tokens | record ends << 16, consumed and
// the depth flags.  kWrite true: the tokens, from the scanned counts.
template <bool kWrite>
__global__ void __launch_bounds__(kJBlock)
json_tokens_kernel(const uint8_t* data, int64_t n, const uint16_t* structmask,
                   const int32_t* tile_depth_in, const int32_t* tile_tok_base,
                   const int32_t* tile_close_base, int32_t* tile_counts,
                   int64_t T, int32_t* tok_pos, int32_t* tok_meta,
                   int32_t* info) {
  __shared__ int32_t drow[kJWaves], crow[kJWaves];
  const int64_t pos0 = (int64_t)blockIdx.x * kJTile + threadIdx.x * 16;
  const uint32_t m = structmask[(int64_t)blockIdx.x * kJBlock + threadIdx.x];
  Bytes16 b{0, 0};
  if (m && pos0 < n) b = load16(data, n, pos0);
  const uint32_t op = (eq_mask(b, '{') | eq_mask(b, '[')) & m;
  const uint32_t cl = (eq_mask(b, '}') | eq_mask(b, ']')) & m;
  int total;
  const int d = tile_depth_in[blockIdx.x] +
                block_excl(__popc(op) - __popc(cl), drow, &total);
  int ncloses = 0;
  int32_t err = 0, consumed = 0;
  const int ntok = walk_tokens<false>(b, m, d, pos0, 0, 0, 0, nullptr, nullptr,
                                      &ncloses, &err, &consumed);
  const int before = block_excl(ntok | (ncloses << 16), crow, &total);
  if (!kWrite) {
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
    for (int off = WAVE / 2; off; off >>= 1) {
      consumed = max(consumed, __shfl_xor(consumed, off, WAVE));
      err |= __shfl_xor(err, off, WAVE);
    }
    if (lane_id() == 0) {
      if (consumed) atomicMax(info + kJConsumed, consumed);
      if (err) atomicOr(info + kJErr, err);
    }
  } else {
    walk_tokens<true>(b, m, d, pos0,
                      (int64_t)tile_tok_base[blockIdx.x] + (before & 0xFFFF),
                      (uint32_t)tile_close_base[blockIdx.x] + (before >> 16),
                      T, tok_pos, tok_meta, &ncloses, &err, &consumed);
  }
}

// ---------------------------------------------------------------------------
// fields: grammar of the token sequence, keys -> columns
// ---------------------------------------------------------------------------
DEV_INLINE bool is_space(uint32_t c) {
  return c == ' ' || c == '\t' || c == '\r' || c == '\n';
}

DEV_INLINE bool all_space(const uint8_t* data, int32_t a, int32_t e) {
  for (; a < e; ++a)
    if (!is_space(data[a])) return false;
  return true;
}

DEV_INLINE void trim(const uint8_t* data, int32_t* a, int32_t* e) {
  while (*a < *e && is_space(data[*a])) ++*a;
  while (*e > *a && is_space(data[*e - 1])) --*e;
}

// keys: [0] ncols, [1] bytes of all names, then kKeyHash slots (column or
// -1; FNV-1a, linear probing), ncols + 1 offsets, and the names' bytes
__global__ void __launch_bounds__(kJBlock)
json_fields_kernel(const uint8_t* data, const int32_t* tok_pos,
                   const int32_t* tok_meta, int64_t T, int32_t consumed,
                   const int32_t* keys, int key_words, int ncols, int64_t R,
                   int32_t* field_tok, int32_t* row_end, int32_t* info) {
  __shared__ int32_t skeys[kKeyWords];
  for (int i = threadIdx.x; i < key_words; i += blockDim.x) skeys[i] = keys[i];
  __syncthreads();
  const int32_t* table = skeys + 2;
  const int32_t* offs = table + kKeyHash;
  const uint8_t* names = (const uint8_t*)(offs + ncols + 1);

  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x; t0 < T; t0 += stride) {
    const int64_t t = t0 + threadIdx.x;
    int32_t err = 0, rows = 0;
    const int32_t p = t < T ? tok_pos[t] : consumed;
    if (p < consumed) {
      const uint32_t meta = (uint32_t)tok_meta[t];
      const int kind = meta & 3;
      const int64_t row = meta >> 2;
      const int32_t prev = t ? tok_pos[t - 1] : -1;
      int32_t next = consumed;
      int nk = -1;  // kind of the next token before `consumed`
      if (t + 1 < T && tok_pos[t + 1] < consumed) {
        next = tok_pos[t + 1];
        nk = tok_meta[t + 1] & 3;
      }
      if (kind == 0) {
        if (nk != 1 && nk != 3) err |= kJIrregular;
        if (!all_space(data, prev + 1, p)) err |= kJIrregular;
        if (nk == 3 && !all_space(data, p + 1, next)) err |= kJIrregular;
      } else if (kind == 2) {
        if (nk != 1) err |= kJIrregular;
      } else if (kind == 3) {
        rows = (int32_t)row + 1;
        if (row < R) row_end[row] = p;
        if (nk < 0 && !all_space(data, p + 1, consumed)) err |= kJIrregular;
      } else {
        if (nk != 2 && nk != 3) err |= kJIrregular;
        int32_t a = prev + 1, e = p;
        trim(data, &a, &e);
        if (e - a < 2 || data[a] != '"' || data[e - 1] != '"') {
          err |= kJIrregular;
        } else {
          ++a, --e;
          uint32_t h = 2166136261u;
          bool escaped = false;
          for (int32_t q = a; q < e; ++q) {
            const uint32_t c = data[q];
            if (c == '\\') escaped = true;
            if (c == '"') err |= kJIrregular;
            h = (h ^ c) * 16777619u;
          }
          int col = -1;
          if (escaped) {
            err |= kJKeyEscape;
          } else {
            uint32_t slot = h & (kKeyHash - 1);
            for (int probe = 0; probe < kKeyHash; ++probe) {
              const int c = table[slot];
              if (c < 0 || c >= ncols) break;
              if (offs[c + 1] - offs[c] == e - a && offs[c] >= 0 &&
                  offs[c + 1] <= kMaxKeyBytes) {
                const uint8_t* name = names + offs[c];
                int32_t q = 0;
                while (q < e - a && name[q] == data[a + q]) ++q;
                if (q == e - a) {
                  col = c;
                  break;
                }
              }
              slot = (slot + 1) & (kKeyHash - 1);
            }
            if (col < 0) err |= kJUnknownKey;
          }
          if (col >= 0 && row < R &&
              atomicCAS(field_tok + col * R + row, -1, (int32_t)t) != -1)
            err |= kJDupKey;
        }
      }
    }
    for (int off = WAVE / 2; off; off >>= 1) {
      rows = max(rows, __shfl_xor(rows, off, WAVE));
      err |= __shfl_xor(err, off, WAVE);
    }
    if (lane_id() == 0) {
      if (rows) atomicMax(info + kJRows, rows);
      if (err) atomicOr(info + kJErr, err);
    }
  }
}

// ---------------------------------------------------------------------------
// values
// ---------------------------------------------------------------------------
DEV_INLINE int hex4(const uint8_t* d) {
  int v = 0;
  for (int i = 0; i < 4; ++i) {
    const int c = d[i];
    const int h = c >= '0' && c <= '9' ? c - '0'
                  : (c | 0x20) >= 'a' && (c | 0x20) <= 'f' ? (c | 0x20) - 'a' + 10
                                                           : -1;
    if (h < 0) return -1;
    v = v * 16 + h;
  }
  return v;
}

// The escape whose '\' is data[p], inside a string that ends at `end`:
// `in` bytes of text (1 .. 12) become `out` bytes, packed low byte first.
// `low`: a \uDC00..\uDFFF on its own, good only as the second half of a pair.
struct Escape {
  int in, out;
  uint32_t bytes;
  bool bad, low;
};

DEV_INLINE Escape decode_escape(const uint8_t* data, int32_t p, int32_t end) {
  Escape r{2, 1, '?', false, false};
  if (p + 1 >= end) {
    r.in = 1, r.bad = true;
    return r;
  }
  switch (data[p + 1]) {
    case '"': r.bytes = '"'; return r;
    case '\\': r.bytes = '\\'; return r;
    case '/': r.bytes = '/'; return r;
    case 'b': r.bytes = '\b'; return r;
    case 'f': r.bytes = '\f'; return r;
    case 'n': r.bytes = '\n'; return r;
    case 'r': r.bytes = '\r'; return r;
    case 't': r.bytes = '\t'; return r;
    case 'u': break;
    default: r.bad = true; return r;
  }
  int h = p + 6 <= end ? hex4(data + p + 2) : -1;
  if (h < 0) {
    r.bad = true;
    return r;
  }
  r.in = 6;
  uint32_t cp = h;
  if (h >= 0xD800 && h < 0xDC00) {
    int l = p + 12 <= end && data[p + 6] == '\\' && data[p + 7] == 'u'
                ? hex4(data + p + 8) : -1;
    if (l < 0xDC00 || l >= 0xE000) {
      r.bad = true;  // a lone high surrogate
    } else {
      cp = 0x10000 + ((uint32_t)(h - 0xD800) << 10) + (l - 0xDC00);
      r.in = 12;
    }
  } else if (h >= 0xDC00 && h < 0xE000) {
    r.low = true;
  }
  if (cp < 0x80) {
    r.out = 1, r.bytes = cp;
  } else if (cp < 0x800) {
    r.out = 2, r.bytes = (0xC0 | cp >> 6) | (0x80 | (cp & 0x3F)) << 8;
  } else if (cp < 0x10000) {
    r.out = 3, r.bytes = (0xE0 | cp >> 12) | (0x80 | (cp >> 6 & 0x3F)) << 8 |
                         (0x80 | (cp & 0x3F)) << 16;
  } else {
    r.out = 4, r.bytes = (0xF0 | cp >> 18) | (0x80 | (cp >> 12 & 0x3F)) << 8 |
                         (0x80 | (cp >> 6 & 0x3F)) << 16 |
                         (0x80u | (cp & 0x3F)) << 24;
  }
  return r;
}

// String content [a, e) walked by one thread: its unescaped length, and with
// kWrite its bytes at out[o ..), kept inside [0, total).
template <bool kWrite>
DEV_INLINE int64_t thread_string(const uint8_t* data, int32_t a, int32_t e,
                                 int64_t o, int64_t total, uint8_t* out,
                                 int32_t* err, bool* escapes) {
  int64_t len = 0;
  for (int32_t p = a; p < e;) {
    const uint8_t c = data[p];
    if (c != '\\') {
      if (c == '"') *err |= kJIrregular;
      if (kWrite && o + len >= 0 && o + len < total) out[o + len] = c;
      ++len, ++p;
      continue;
    }
    *escapes = true;
    const Escape x = decode_escape(data, p, e);
    if (x.bad || x.low) *err |= kJBadEscape;
    if (kWrite)
      for (int q = 0; q < x.out; ++q)
        if (o + len + q >= 0 && o + len + q < total)
          out[o + len + q] = (uint8_t)(x.bytes >> (8 * q));
    len += x.out;
    p += x.in;
  }
  return len;
}

// The same for a long string, by all 64 lanes of the wave, 64 bytes per step.
// The '\' that start an escape are the ballot of '\' minus the escaped ones
// (escaped_mask's arithmetic on 64 bits, the add's carry handed to the next
// step).  Each start decodes its escape and drops in - out bytes at its own
// position; a byte's slot is its index minus the drops before it.
template <bool kWrite>
DEV_INLINE int64_t wave_string(const uint8_t* data, int32_t sa, int32_t se,
                               int64_t so, int64_t total, uint8_t* out,
                               int32_t* err, bool* escapes) {
  const int lane = lane_id();
  const uint64_t even = 0x5555555555555555ull;
  uint64_t prev_escaped = 0, prev_high = 0, cover_in = 0;
  int dropped = 0;
  for (int32_t p0 = sa; p0 < se; p0 += WAVE) {
    const int32_t p = p0 + lane;
    const bool live = p < se;
    const uint8_t ch = live ? data[p] : 0;
    const uint64_t bs = __ballot(live && ch == '\\') & ~prev_escaped;
    const uint64_t follows = (bs << 1) | prev_escaped;
    const uint64_t odd_starts = bs & ~even & ~follows;
    const uint64_t sum = odd_starts + bs;
    const uint64_t escaped = (even ^ (sum << 1)) & follows;
    prev_escaped = sum < bs ? 1 : 0;
    if (bs | follows) *escapes = true;
    if (__ballot(live && ch == '"') & ~escaped) *err |= kJIrregular;

    bool start = (bs & ~escaped) >> lane & 1;
    Escape x{0, 0, 0, false, false};
    if (start) x = decode_escape(data, p, se);
    // the second half of a surrogate pair sits 6 bytes behind its first
    const uint64_t high = __ballot(start && x.in == 12);
    const uint64_t second = (high << 6) | (prev_high >> 58);
    prev_high = high;
    if (start && x.low) {
      if (second >> lane & 1) start = false;
      else x.bad = true;
    }
    if (start && x.bad) *err |= kJBadEscape;
    const int drop = start ? x.in - x.out : 0;
    int run = drop;  // inclusive prefix over the wave
    for (int off = 1; off < WAVE; off <<= 1) {
      int t = __shfl_up(run, off, WAVE);
      if (lane >= off) run += t;
    }
    if (kWrite) {
      // bytes behind a start that belong to its escape write nothing
      const uint64_t s2 = __ballot(start && x.in == 2);
      const uint64_t s6 = __ballot(start && x.in == 6);
      uint64_t cover = cover_in | s2 << 1, over = s2 >> 63;
      for (int k = 1; k < 6; ++k) cover |= s6 << k, over |= s6 >> (64 - k);
      for (int k = 1; k < 12; ++k) cover |= high << k, over |= high >> (64 - k);
      cover_in = over;
      const int64_t at = so + (p - sa) - (dropped + run - drop);
      if (live && start) {
        for (int q = 0; q < x.out; ++q)
          if (at + q >= 0 && at + q < total)
            out[at + q] = (uint8_t)(x.bytes >> (8 * q));
      } else if (live && !(cover >> lane & 1) && at >= 0 && at < total) {
        out[at] = ch;
      }
    }
    dropped += __shfl(run, WAVE - 1, WAVE);
  }
  return (int64_t)(se - sa) - dropped;
}

DEV_INLINE bool is_digit(uint32_t c) { return c >= '0' && c <= '9'; }

// -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?
DEV_INLINE bool number_ok(const uint8_t* d, int32_t p, int32_t e) {
  if (p < e && d[p] == '-') ++p;
  if (p >= e || !is_digit(d[p])) return false;
  if (d[p] == '0') ++p;
  else while (p < e && is_digit(d[p])) ++p;
  if (p < e && d[p] == '.') {
    const int32_t s = ++p;
    while (p < e && is_digit(d[p])) ++p;
    if (p == s) return false;
  }
  if (p < e && (d[p] | 0x20) == 'e') {
    ++p;
    if (p < e && (d[p] == '+' || d[p] == '-')) ++p;
    const int32_t s = p;
    while (p < e && is_digit(d[p])) ++p;
    if (p == s) return false;
  }
  return p == e;
}

DEV_INLINE bool literal(const uint8_t* d, int32_t a, int32_t e, const char* s,
                        int len) {
  if (e - a != len) return false;
  for (int i = 0; i < len; ++i)
    if (d[a + i] != (uint8_t)s[i]) return false;
  return true;
}

// blockIdx.y is the column, the x dimension strides over rows.  raw_start and
// raw_len: the trimmed value text (a string's with its quotes); ulen: a
// string's unescaped content length, 0 for every other kind; seen[col]: bit k
// for a value of kind k, bit 8 for a string with a backslash.
__global__ void __launch_bounds__(kJBlock)
json_values_kernel(const uint8_t* data, const int32_t* tok_pos, int64_t T,
                   const int32_t* field_tok, int64_t R, const int32_t* row_end,
                   int64_t nrows, uint8_t* kinds, int64_t* raw_start,
                   int64_t* raw_len, int64_t* ulen, int32_t* seen,
                   int32_t* info) {
  const int64_t j = blockIdx.y;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r0 = (int64_t)blockIdx.x * blockDim.x; r0 < nrows;
       r0 += stride) {
    const int64_t r = r0 + threadIdx.x;
    int32_t a = 0, e = 0, err = 0, record = 0;
    int kind = kNull;
    int64_t len = 0;
    bool escapes = false, is_long = false;
    if (r < nrows) {
      const int32_t t = field_tok[j * R + r];
      if (t >= 0 && t + 1 < T) {
        a = tok_pos[t] + 1, e = tok_pos[t + 1];
        trim(data, &a, &e);
        const uint32_t c = a < e ? data[a] : 0;
        if (a >= e) {
          err |= kJIrregular;
        } else if (c == '"') {
          kind = kString;
          if (e - a < 2 || data[e - 1] != '"') err |= kJIrregular;
          else if (e - a - 2 >= kLongValue) is_long = true;
          else len = thread_string<false>(data, a + 1, e - 1, 0, 0, nullptr,
                                          &err, &escapes);
        } else if (c == '{' || c == '[') {
          kind = kNested;
        } else if (c == 't' || c == 'f' || c == 'n') {
          kind = c == 't' ? kTrue : c == 'f' ? kFalse : kNull;
          if (!literal(data, a, e, c == 't' ? "true" : c == 'f' ? "false"
                                                                 : "null",
                       c == 'f' ? 5 : 4))
            err |= kJIrregular;
        } else {
          kind = kNumber;
          if (!number_ok(data, a, e)) err |= kJIrregular;
        }
      }
      if (j == 0) record = row_end[r] - (r ? row_end[r - 1] : -1);
    }
    for (uint64_t todo = __ballot(is_long); todo; todo &= todo - 1) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      const int32_t sa = __shfl(a, src, WAVE) + 1;
      const int32_t se = __shfl(e, src, WAVE) - 1;
      int32_t werr = 0;
      bool wesc = false;
      const int64_t wlen =
          wave_string<false>(data, sa, se, 0, 0, nullptr, &werr, &wesc);
      for (int off = WAVE / 2; off; off >>= 1)
        werr |= __shfl_xor(werr, off, WAVE);
      if (lane_id() == src) len = wlen, err |= werr, escapes = wesc;
    }
    int32_t bits = 0;
    if (r < nrows) {
      kinds[j * nrows + r] = (uint8_t)kind;
      raw_start[j * nrows + r] = a;
      raw_len[j * nrows + r] = kind == kNull ? 0 : e - a;
      ulen[j * nrows + r] = len;
      bits = 1 << kind | (escapes ? 256 : 0);
    }
    for (int off = WAVE / 2; off; off >>= 1) {
      bits |= __shfl_xor(bits, off, WAVE);
      err |= __shfl_xor(err, off, WAVE);
      record = max(record, __shfl_xor(record, off, WAVE));
    }
    if (lane_id() == 0) {
      if (bits) atomicOr(seen + j, bits);
      if (err) atomicOr(info + kJErr, err);
      if (record) atomicMax(info + kJMaxRecord, record);
    }
  }
}

// one string column with escapes: row r's content to out[out_offs[r] ..)
__global__ void __launch_bounds__(kJBlock)
json_unescape_kernel(const uint8_t* data, int64_t n, const uint8_t* kinds,
                     const int64_t* raw_start, const int64_t* raw_len,
                     int64_t nrows, const int64_t* out_offs, int64_t total,
                     uint8_t* out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r0 = (int64_t)blockIdx.x * blockDim.x; r0 < nrows;
       r0 += stride) {
    const int64_t r = r0 + threadIdx.x;
    int32_t a = 0, e = 0, err = 0;
    int64_t o = 0;
    bool escapes = false;
    if (r < nrows && kinds[r] == kString) {
      const int64_t s = raw_start[r], l = raw_len[r];
      if (s >= 0 && l >= 2 && s + l <= n) {
        a = (int32_t)s + 1, e = (int32_t)(s + l) - 1;
        o = out_offs[r];
      }
    }
    const bool is_long = e - a >= kLongValue;
    if (!is_long)
      thread_string<true>(data, a, e, o, total, out, &err, &escapes);
    for (uint64_t todo = __ballot(is_long); todo; todo &= todo - 1) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      wave_string<true>(data, __shfl(a, src, WAVE), __shfl(e, src, WAVE),
                        __shfl(o, src, WAVE), total, out, &err, &escapes);
    }
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
static int64_t check_json_chunk(const char* who, const Tensor& data) {
  TORCH_CHECK(data.is_cuda(), who, ": data must be on a GPU device");
  check_tensor(who, "data", data, torch::kUInt8, data.device());
  TORCH_CHECK(data.dim() == 1 && data.numel() < (int64_t)INT_MAX, who,
              ": data must be one chunk of fewer than 2^31 bytes");
  TORCH_CHECK(data.numel() == 0 || (uintptr_t)data.data_ptr() % 16 == 0, who,
              ": data must be 16-byte aligned");
  return data.numel();
}

// a 1-D tensor of `numel` entries (at least, with at_least) on `dev`
static void check_vec(const char* who, const char* name, const Tensor& t,
                      torch::ScalarType dtype, const torch::Device& dev,
                      int64_t numel) {
  check_tensor(who, name, t, dtype, dev);
  TORCH_CHECK(t.numel() == numel, who, ": ", name, " must have ", numel,
              " entries, got ", t.numel());
}

Tensor json_keys(std::vector<std::string> names) {
  int64_t nbytes = 0;
  for (auto& s : names) nbytes += (int64_t)s.size();
  TORCH_CHECK(!names.empty() && (int64_t)names.size() <= kMaxKeys &&
                  nbytes <= kMaxKeyBytes,
              "json_keys: 1 .. ", kMaxKeys, " names of at most ", kMaxKeyBytes,
              " bytes in all");
  const int ncols = (int)names.size();
  auto blob = torch::zeros({2 + kKeyHash + ncols + 1 + (nbytes + 3) / 4},
                           torch::kInt32);
  int32_t* w = blob.data_ptr<int32_t>();
  w[0] = ncols, w[1] = (int32_t)nbytes;
  int32_t* table = w + 2;
  int32_t* offs = table + kKeyHash;
  uint8_t* bytes = (uint8_t*)(offs + ncols + 1);
  std::fill(table, table + kKeyHash, -1);
  for (int c = 0; c < ncols; ++c) {
    uint32_t h = 2166136261u;
    for (unsigned char ch : names[c]) h = (h ^ ch) * 16777619u;
    uint32_t slot = h & (kKeyHash - 1);
    while (table[slot] >= 0) slot = (slot + 1) & (kKeyHash - 1);
    table[slot] = c;
    offs[c + 1] = offs[c] + (int32_t)names[c].size();
    std::copy(names[c].begin(), names[c].end(), bytes + offs[c]);
  }
  return blob;
}

std::vector<Tensor> json_structure(Tensor data) {
  const int64_t n = check_json_chunk("json_structure", data);
  auto dev = data.device();
  auto i32 = torch::dtype(torch::kInt32).device(dev);
  const int64_t ntiles = (n + kJTile - 1) / kJTile;
  auto info = torch::zeros({kJInfoLen}, i32);
  auto mask = torch::empty({ntiles * kJBlock},
                           torch::dtype(torch::kInt16).device(dev));
  auto none = torch::empty({0}, i32);
  if (n == 0) return {mask, none, none, none, info};
  const uint8_t* d = data.data_ptr<uint8_t>();
  int32_t* inf = info.data_ptr<int32_t>();
  auto parity = torch::empty({ntiles}, i32);
  auto depth = torch::empty({ntiles}, i32);
  auto counts = torch::empty({ntiles}, i32);
  hipLaunchKernelGGL(json_summary_kernel, dim3((unsigned)ntiles),
                     dim3(kJBlock), 0, cur_stream(), d, n,
                     parity.data_ptr<int32_t>(), inf);
  auto incl = torch::cumsum(parity, 0);
  auto parity_in = ((incl - parity) & 1).to(torch::kInt32);
  info.select(0, kJEndParity).copy_(incl[ntiles - 1] & 1);
  hipLaunchKernelGGL(json_classify_kernel, dim3((unsigned)ntiles),
                     dim3(kJBlock), 0, cur_stream(), d, n,
                     parity_in.data_ptr<int32_t>(),
                     (uint16_t*)mask.data_ptr<int16_t>(),
                     depth.data_ptr<int32_t>(), inf);
  auto depth_in = (torch::cumsum(depth, 0) - depth).to(torch::kInt32);
  hipLaunchKernelGGL(json_tokens_kernel<false>, dim3((unsigned)ntiles),
                     dim3(kJBlock), 0, cur_stream(), d, n,
                     (const uint16_t*)mask.data_ptr<int16_t>(),
                     depth_in.data_ptr<int32_t>(), (const int32_t*)nullptr,
                     (const int32_t*)nullptr, counts.data_ptr<int32_t>(),
                     (int64_t)0, (int32_t*)nullptr, (int32_t*)nullptr, inf);
  auto toks = counts & 0xFFFF, closes = counts.bitwise_right_shift(16);
  auto tok_run = torch::cumsum(toks, 0), close_run = torch::cumsum(closes, 0);
  info.select(0, kJTokens).copy_(tok_run[ntiles - 1]);
  info.select(0, kJCloses).copy_(close_run[ntiles - 1]);
  return {mask, depth_in, (tok_run - toks).to(torch::kInt32),
          (close_run - closes).to(torch::kInt32), info};
}

Tensor json_tokens(Tensor data, Tensor structmask, Tensor depth_in,
                   Tensor tok_base, Tensor close_base, int64_t T) {
  const int64_t n = check_json_chunk("json_tokens", data);
  auto dev = data.device();
  const int64_t ntiles = (n + kJTile - 1) / kJTile;
  check_vec("json_tokens", "structmask", structmask, torch::kInt16, dev,
            ntiles * kJBlock);
  check_vec("json_tokens", "depth_in", depth_in, torch::kInt32, dev, ntiles);
  check_vec("json_tokens", "tok_base", tok_base, torch::kInt32, dev, ntiles);
  check_vec("json_tokens", "close_base", close_base, torch::kInt32, dev,
            ntiles);
  TORCH_CHECK(T >= 0 && T <= n, "json_tokens: need 0 <= T <= n, got ", T);
  auto tokens = torch::empty({2, T}, torch::dtype(torch::kInt32).device(dev));
  if (T == 0) return tokens;
  hipLaunchKernelGGL(json_tokens_kernel<true>, dim3((unsigned)ntiles),
                     dim3(kJBlock), 0, cur_stream(), data.data_ptr<uint8_t>(),
                     n, (const uint16_t*)structmask.data_ptr<int16_t>(),
                     depth_in.data_ptr<int32_t>(),
                     tok_base.data_ptr<int32_t>(),
                     close_base.data_ptr<int32_t>(), (int32_t*)nullptr, T,
                     tokens.data_ptr<int32_t>(),
                     tokens.data_ptr<int32_t>() + T, (int32_t*)nullptr);
  return tokens;
}

// tokens must be json_tokens' for this chunk: positions in [0, n), ascending
static int64_t check_tokens(const char* who, const Tensor& tokens,
                            const Tensor& data) {
  check_tensor(who, "tokens", tokens, torch::kInt32, data.device());
  TORCH_CHECK(tokens.dim() == 2 && tokens.size(0) == 2, who,
              ": tokens must be int32 [2, T]");
  return tokens.size(1);
}


std::vector<Tensor> json_fields(Tensor data, Tensor tokens, int64_t consumed,
                                int64_t R, Tensor keys, int64_t ncols,
                                Tensor info) {
  const int64_t n = check_json_chunk("json_fields", data);
  auto dev = data.device();
  const int64_t T = check_tokens("json_fields", tokens, data);
  check_tensor("json_fields", "keys", keys, torch::kInt32, dev);
  check_vec("json_fields", "info", info, torch::kInt32, dev, kJInfoLen);
  TORCH_CHECK(ncols >= 1 && ncols <= kMaxKeys && keys.dim() == 1 &&
                  keys.numel() >= 2 + kKeyHash + ncols + 1 &&
                  keys.numel() <= kKeyWords,
              "json_fields: keys must be json_keys' tensor for ", ncols,
              " names");
  TORCH_CHECK(consumed >= 0 && consumed <= n && R >= 0 && R <= T,
              "json_fields: need 0 <= consumed <= n and 0 <= R <= T");
  auto i32 = torch::dtype(torch::kInt32).device(dev);
  auto field_tok = torch::full({ncols, R}, -1, i32);
  auto row_end = torch::zeros({R}, i32);
  if (T == 0) return {field_tok, row_end};
  hipLaunchKernelGGL(json_fields_kernel, dim3(grid_1d(T, kJBlock)),
                     dim3(kJBlock), 0, cur_stream(), data.data_ptr<uint8_t>(),
                     tokens.data_ptr<int32_t>(),
                     tokens.data_ptr<int32_t>() + T, T, (int32_t)consumed,
                     keys.data_ptr<int32_t>(), (int)keys.numel(), (int)ncols,
                     R, field_tok.data_ptr<int32_t>(),
                     row_end.data_ptr<int32_t>(), info.data_ptr<int32_t>());
  return {field_tok, row_end};
}

std::vector<Tensor> json_values(Tensor data, Tensor tokens, Tensor field_tok,
                                Tensor row_end, int64_t nrows, Tensor info) {
  check_json_chunk("json_values", data);
  auto dev = data.device();
  const int64_t T = check_tokens("json_values", tokens, data);
  check_tensor("json_values", "field_tok", field_tok, torch::kInt32, dev);
  check_tensor("json_values", "row_end", row_end, torch::kInt32, dev);
  check_vec("json_values", "info", info, torch::kInt32, dev, kJInfoLen);
  TORCH_CHECK(field_tok.dim() == 2 && row_end.dim() == 1 &&
                  field_tok.size(1) == row_end.numel() &&
                  field_tok.size(0) >= 1 && field_tok.size(0) <= kMaxKeys,
              "json_values: field_tok [ncols, R] and row_end [R] must be "
              "json_fields'");
  const int64_t ncols = field_tok.size(0), R = field_tok.size(1);
  TORCH_CHECK(nrows >= 0 && nrows <= R, "json_values: need 0 <= nrows <= ", R);
  auto i64 = torch::dtype(torch::kInt64).device(dev);
  auto kinds = torch::empty({ncols, nrows},
                            torch::dtype(torch::kUInt8).device(dev));
  auto raw_start = torch::empty({ncols, nrows}, i64);
  auto raw_len = torch::empty({ncols, nrows}, i64);
  auto ulen = torch::empty({ncols, nrows}, i64);
  auto seen = torch::zeros({ncols}, torch::dtype(torch::kInt32).device(dev));
  if (nrows == 0) return {kinds, raw_start, raw_len, ulen, seen};
  int gx = std::min(grid_1d(nrows, kJBlock), 1024);
  hipLaunchKernelGGL(json_values_kernel, dim3(gx, (unsigned)ncols),
                     dim3(kJBlock), 0, cur_stream(), data.data_ptr<uint8_t>(),
                     tokens.data_ptr<int32_t>(), T,
                     field_tok.data_ptr<int32_t>(), R,
                     row_end.data_ptr<int32_t>(), nrows,
                     kinds.data_ptr<uint8_t>(), raw_start.data_ptr<int64_t>(),
                     raw_len.data_ptr<int64_t>(), ulen.data_ptr<int64_t>(),
                     seen.data_ptr<int32_t>(), info.data_ptr<int32_t>());
  return {kinds, raw_start, raw_len, ulen, seen};
}

Tensor json_extract(Tensor data, Tensor kinds, Tensor raw_start,
                    Tensor raw_len, Tensor out_offsets, int64_t total,
                    bool unescape) {
  const int64_t n = check_json_chunk("json_extract", data);
  auto dev = data.device();
  check_tensor("json_extract", "out_offsets", out_offsets, torch::kInt64, dev);
  TORCH_CHECK(out_offsets.dim() == 1 && out_offsets.numel() >= 1,
              "json_extract: out_offsets must be [nrows + 1]");
  const int64_t nrows = out_offsets.numel() - 1;
  check_vec("json_extract", "kinds", kinds, torch::kUInt8, dev, nrows);
  check_vec("json_extract", "raw_start", raw_start, torch::kInt64, dev, nrows);
  check_vec("json_extract", "raw_len", raw_len, torch::kInt64, dev, nrows);
  TORCH_CHECK(total >= 0 && total <= n,
              "json_extract: need 0 <= total <= n, got ", total);
  auto out = torch::empty({total}, torch::dtype(torch::kUInt8).device(dev));
  if (total == 0 || nrows == 0) return out;
  if (!unescape) {
    // raw_start is where the copy begins: the caller has stepped over a
    // string's opening quote
    launch_copy_segments(data.data_ptr<uint8_t>(), n,
                         raw_start.data_ptr<int64_t>(),
                         out_offsets.data_ptr<int64_t>(), nrows, total,
                         out.data_ptr<uint8_t>());
  } else {
    hipLaunchKernelGGL(json_unescape_kernel, dim3(grid_1d(nrows, kJBlock)),
                       dim3(kJBlock), 0, cur_stream(),
                       data.data_ptr<uint8_t>(), n, kinds.data_ptr<uint8_t>(),
                       raw_start.data_ptr<int64_t>(),
                       raw_len.data_ptr<int64_t>(), nrows,
                       out_offsets.data_ptr<int64_t>(), total,
                       out.data_ptr<uint8_t>());
  }
  return out;
}
