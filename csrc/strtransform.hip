// Text cleanup over Arrow offsets+bytes (gfx950): strip, right, reverse and
// the ASCII normalizer.  strip and right are a bounds kernel (one thread per
// row) followed by the shared ragged copy of strings.hip; reverse is
// byte-parallel; normalize runs one 64-lane wave per row in two passes.
#include "common.h"
#include "host_args.h"
#include "api.h"

// ASCII part of Python's str.isspace: U+0009-000D, U+001C-001F, U+0020
DEV_INLINE bool ascii_space(uint8_t c) {
  return (c >= 0x09 && c <= 0x0D) || (c >= 0x1C && c <= 0x20);
}

// Bytes of the str.isspace character that starts at s[p], 0 when there is
// none.  p < end; nothing at or past `end` is read, so a sequence cut short
// by the row's end is no space.
DEV_INLINE int space_at(const uint8_t* s, int64_t p, int64_t end) {
  uint8_t c = s[p];
  if (c < 0x80) return ascii_space(c) ? 1 : 0;
  if (c == 0xC2)                                    // U+0085, U+00A0
    return (p + 1 < end && (s[p + 1] == 0x85 || s[p + 1] == 0xA0)) ? 2 : 0;
  if (c < 0xE1 || c > 0xE3 || p + 2 >= end) return 0;
  uint8_t d = s[p + 1], e = s[p + 2];
  bool hit;
  if (c == 0xE1) {
    hit = d == 0x9A && e == 0x80;                   // U+1680
  } else if (c == 0xE2) {
    hit = (d == 0x80 && ((e >= 0x80 && e <= 0x8A) ||  // U+2000-200A
                         e == 0xA8 || e == 0xA9 ||    // U+2028, U+2029
                         e == 0xAF)) ||               // U+202F
          (d == 0x81 && e == 0x9F);                 // U+205F
  } else {
    hit = d == 0x80 && e == 0x80;                   // U+3000
  }
  return hit ? 3 : 0;
}

// Bytes of the str.isspace character that ends just before s[end], 0 when
// there is none.  lo < end; nothing before s[lo] is read.  C2 and E1-E3 are
// lead bytes, so a hit one or two bytes back is a whole character.
DEV_INLINE int space_before(const uint8_t* s, int64_t lo, int64_t end) {
  if (s[end - 1] < 0x80) return ascii_space(s[end - 1]) ? 1 : 0;
  if (end - 2 >= lo && space_at(s, end - 2, end) == 2) return 2;
  if (end - 3 >= lo && space_at(s, end - 3, end) == 3) return 3;
  return 0;
}

// mode: 0 = both sides, 1 = left, 2 = right
__global__ void strip_bounds_kernel(const int64_t* offs, const uint8_t* bytes,
                                    int64_t n, int mode, int64_t* src_start,
                                    int64_t* out_len) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t a = offs[i], len = offs[i + 1] - a;
    const uint8_t* s = bytes + a;
    int64_t lo = 0, hi = len;
    if (mode != 2) {
      while (lo < hi) {
        int w = space_at(s, lo, hi);
        if (!w) break;
        lo += w;
      }
    }
    if (mode != 1) {
      while (lo < hi) {
        int w = space_before(s, lo, hi);
        if (!w) break;
        hi -= w;
      }
    }
    src_start[i] = a + lo;
    out_len[i] = hi - lo;
  }
}

// The last `k` code points of each row (k >= 0): walk back from the row's
// end over `k` bytes that are not 10xxxxxx continuation bytes.
__global__ void right_bounds_kernel(const int64_t* offs, const uint8_t* bytes,
                                    int64_t n, int64_t k, int64_t* src_start,
                                    int64_t* out_len) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t a = offs[i], len = offs[i + 1] - a;
    const uint8_t* s = bytes + a;
    int64_t j = len, cnt = 0;
    while (cnt < k && j > 0) {
      --j;
      if ((s[j] & 0xC0) != 0x80) ++cnt;
    }
    src_start[i] = a + j;
    out_len[i] = len - j;
  }
}

// {offsets, bytes} of the rows [src_start[i], src_start[i] + lens[i])
static std::vector<Tensor> copy_rows(const StrCol& c, const Tensor& bytes,
                                     const Tensor& src_start,
                                     const Tensor& lens) {
  auto [out_off, total] = offsets_from_lens(lens);
  auto out = torch::empty({total}, bytes.options());
  launch_copy_segments(c.bytes, c.nbytes, src_start.data_ptr<int64_t>(),
                       out_off.data_ptr<int64_t>(), c.n, total,
                       out.data_ptr<uint8_t>());
  return {out_off, out};
}

std::vector<Tensor> str_strip(Tensor offsets, Tensor bytes, int64_t mode) {
  TORCH_CHECK(mode >= 0 && mode <= 2, "str_strip: mode must be 0, 1 or 2, got ",
              mode);
  StrCol c = check_strcol("str_strip", offsets, bytes);
  auto opts64 = torch::dtype(torch::kInt64).device(offsets.device());
  auto src_start = torch::empty({c.n}, opts64);
  auto lens = torch::empty({c.n}, opts64);
  int block = 256;
  if (c.n > 0)
    hipLaunchKernelGGL(strip_bounds_kernel, dim3(grid_1d(c.n, block)),
                       dim3(block), 0, cur_stream(), c.offs, c.bytes, c.n,
                       (int)mode, src_start.data_ptr<int64_t>(),
                       lens.data_ptr<int64_t>());
  return copy_rows(c, bytes, src_start, lens);
}

std::vector<Tensor> str_right(Tensor offsets, Tensor bytes, int64_t k) {
  TORCH_CHECK(k >= 0, "str_right: n must be >= 0, got ", k);
  StrCol c = check_strcol("str_right", offsets, bytes);
  auto opts64 = torch::dtype(torch::kInt64).device(offsets.device());
  auto src_start = torch::empty({c.n}, opts64);
  auto lens = torch::empty({c.n}, opts64);
  int block = 256;
  if (c.n > 0)
    hipLaunchKernelGGL(right_bounds_kernel, dim3(grid_1d(c.n, block)),
                       dim3(block), 0, cur_stream(), c.offs, c.bytes, c.n, k,
                       src_start.data_ptr<int64_t>(),
                       lens.data_ptr<int64_t>());
  return copy_rows(c, bytes, src_start, lens);
}

// Reverse by code point, one thread per byte of bytes[base, base + total).
// The thread finds its row by binary search over offs (the last i with
// offs[i] <= g, which steps over empty rows), then its character: it starts
// at the row's first byte or at the nearest byte at or before g that is not
// a continuation byte, and ends before the next such byte or the row's end.
// The character [cs, ce) of the row [a, b) lands at a + (b - ce), so every
// row is permuted onto itself.
__global__ void reverse_kernel(const int64_t* offs, const uint8_t* bytes,
                               int64_t n, int64_t base, int64_t total,
                               uint8_t* out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    int64_t g = base + t;
    int64_t lo = 0, hi = n;  // offs[lo] <= g < offs[hi]
    while (hi - lo > 1) {
      int64_t mid = lo + (hi - lo) / 2;
      if (offs[mid] <= g) lo = mid; else hi = mid;
    }
    int64_t a = offs[lo], b = offs[lo + 1];
    int64_t cs = g, ce = g + 1;
    while (cs > a && (bytes[cs] & 0xC0) == 0x80) --cs;
    while (ce < b && (bytes[ce] & 0xC0) == 0x80) ++ce;
    out[(a - base) + (b - ce) + (g - cs)] = bytes[g];
  }
}

std::vector<Tensor> str_reverse(Tensor offsets, Tensor bytes) {
  StrCol c = check_strcol("str_reverse", offsets, bytes);
  if (c.n == 0)
    return {torch::zeros({1}, offsets.options()),
            torch::empty({0}, bytes.options())};
  // the one sync: where the rows' bytes begin and end
  auto ends = torch::stack({offsets[0], offsets[c.n]}).cpu();
  int64_t base = ends[0].item<int64_t>(), last = ends[1].item<int64_t>();
  TORCH_CHECK(0 <= base && base <= last && last <= c.nbytes,
              "str_reverse: offsets must run inside bytes");
  int64_t total = last - base;
  auto out_off = offsets - base;
  auto out = torch::empty({total}, bytes.options());
  if (total > 0) {
    int block = 256;
    hipLaunchKernelGGL(reverse_kernel, dim3(grid_1d(total, block)),
                       dim3(block), 0, cur_stream(), c.offs, c.bytes, c.n,
                       base, total, out.data_ptr<uint8_t>());
  }
  return {out_off, out};
}

// ---------------------------------------------------------------------------
// normalize, ASCII rows: drop punctuation, fold case, collapse whitespace.
// One wave per row over 64-byte chunks.  Per chunk three ballots class the
// bytes: `sep` (whitespace that is collapsed), `keep` (bytes that are
// written) and, by absence from both, dropped bytes, which leave the state
// alone.  A kept byte is preceded by one ' ' when the nearest earlier byte
// that is not dropped is a separator and some byte was kept before it; that
// byte is the highest bit below the lane in sep | keep, or the carry of the
// chunks before.  WRITE = false counts (pass 1), WRITE = true writes at the
// offsets made from those counts (pass 2).
// ---------------------------------------------------------------------------
constexpr int kNormWaves = 4;  // rows (waves) per 256-thread block

DEV_INLINE bool ascii_word(uint8_t c) {
  return (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') ||
         (c >= 'a' && c <= 'z') || c == '_';
}

template <bool WRITE>
__global__ void __launch_bounds__(kNormWaves * WAVE)
normalize_ascii_kernel(const int64_t* offs, const uint8_t* bytes,
                       const bool* valid, int64_t n, bool remove_punct,
                       bool lowercase, bool white_space, int64_t* out_len,
                       bool* non_ascii, const int64_t* out_off, uint8_t* out) {
  int lane = threadIdx.x & (WAVE - 1);
  uint64_t below = (1ull << lane) - 1;
  int64_t row0 = (int64_t)blockIdx.x * kNormWaves + threadIdx.x / WAVE;
  int64_t row_stride = (int64_t)gridDim.x * kNormWaves;
  // `row` is the same in all 64 lanes, so every branch on it, and on the
  // ballots below, is taken by the whole wave
  for (int64_t row = row0; row < n; row += row_stride) {
    int64_t a = offs[row], len = offs[row + 1] - a;
    int64_t dst = 0;
    if (WRITE) {
      dst = out_off[row];
      if (out_off[row + 1] == dst) continue;  // null, flagged or empty
    } else if (valid && !valid[row]) {
      if (lane == 0) { out_len[row] = 0; non_ascii[row] = false; }
      continue;
    }
    const uint8_t* s = bytes + a;
    int64_t run = 0;           // bytes of output so far
    bool carry_sep = false;    // last byte that was not dropped: a separator
    bool carry_any = false;    // some byte was kept
    bool high = false;
    for (int64_t base = 0; base < len; base += WAVE) {
      bool act = base + lane < len;
      uint8_t c = act ? s[base + lane] : 0;
      if (!WRITE && __ballot(act && c >= 0x80)) { high = true; break; }
      bool ws = act && ascii_space(c);
      bool drop = remove_punct && !ws && !ascii_word(c);
      bool is_sep = ws && white_space;
      bool is_keep = act && !drop && !is_sep;
      uint64_t sep = __ballot(is_sep), keep = __ballot(is_keep);
      uint64_t seen = (sep | keep) & below;
      bool prev_sep =
          seen ? ((sep >> (63 - __clzll((long long)seen))) & 1) : carry_sep;
      bool any_before = carry_any || (keep & below);
      bool space = is_keep && prev_sep && any_before;
      uint64_t spaces = __ballot(space);
      if (WRITE && is_keep) {
        int64_t at = dst + run + __popcll(keep & below) +
                     __popcll(spaces & below);
        if (space) out[at++] = ' ';
        if (lowercase && c >= 'A' && c <= 'Z') c += 32;
        out[at] = c;
      }
      run += __popcll(keep) + __popcll(spaces);
      uint64_t all = sep | keep;
      if (all) carry_sep = (sep >> (63 - __clzll((long long)all))) & 1;
      carry_any = carry_any || keep;
    }
    if (!WRITE && lane == 0) {
      out_len[row] = high ? 0 : run;
      non_ascii[row] = high;
    }
  }
}

std::vector<Tensor> str_normalize_ascii(Tensor offsets, Tensor bytes,
                                        OptTensor valid, bool remove_punct,
                                        bool lowercase, bool white_space) {
  StrCol c = check_strcol("str_normalize_ascii", offsets, bytes);
  auto dev = offsets.device();
  const bool* vptr = check_valid("str_normalize_ascii", valid, c.n, dev);
  auto lens = torch::empty({c.n}, torch::dtype(torch::kInt64).device(dev));
  auto flags = torch::empty({c.n}, torch::dtype(torch::kBool).device(dev));
  int block = kNormWaves * WAVE;
  int grid = grid_1d(c.n, kNormWaves);
  if (c.n > 0)
    hipLaunchKernelGGL(normalize_ascii_kernel<false>, dim3(grid), dim3(block),
                       0, cur_stream(), c.offs, c.bytes, vptr, c.n,
                       remove_punct, lowercase, white_space,
                       lens.data_ptr<int64_t>(), flags.data_ptr<bool>(),
                       (const int64_t*)nullptr, (uint8_t*)nullptr);
  auto [out_off, total] = offsets_from_lens(lens);
  auto out = torch::empty({total}, bytes.options());
  if (total > 0)
    hipLaunchKernelGGL(normalize_ascii_kernel<true>, dim3(grid), dim3(block),
                       0, cur_stream(), c.offs, c.bytes, vptr, c.n,
                       remove_punct, lowercase, white_space,
                       (int64_t*)nullptr, (bool*)nullptr,
                       out_off.data_ptr<int64_t>(), out.data_ptr<uint8_t>());
  return {out_off, out, flags};
}
