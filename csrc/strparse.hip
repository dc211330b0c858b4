// Text <-> value conversion over Arrow offsets+bytes (gfx950): parse
// integers, decimals, floats, dates and datetimes out of a string column, and
// format integers and dates into one.
//
// Parsing: a block of 256 threads owns 256 consecutive rows, whose bytes are
// the one contiguous span [offs[r0], offs[r0 + 256]).  The block copies that
// span into an LDS tile with 16-byte loads (the span's first address aligned
// down to 16; the partial chunks at its head and tail are copied by byte, so
// nothing outside the span is read), then each thread runs its row's state
// machine over LDS.  A block whose span does not fit the tile runs the same
// machine straight over global memory.  Every machine answers a status per
// row: 0 parsed, 1 null, 2 "the host must decide", which it gives whenever it
// is not certain to reproduce Python's answer bit for bit.
#include "common.h"
#include "host_args.h"
#include "api.h"

constexpr int kParseBlock = 256;
constexpr int kParseTile = 16384;  // bytes of LDS per block

#ifndef DAFT_STRPARSE_STAGED
#define DAFT_STRPARSE_STAGED 1     // 0: build with direct reads only
#endif
static bool g_staged = DAFT_STRPARSE_STAGED != 0;

enum : uint8_t { kParsed = 0, kNull = 1, kHost = 2 };

DEV_INLINE bool is_digit(uint8_t c) { return (uint8_t)(c - '0') <= 9; }

// ---------------------------------------------------------------------------
// row machines: status of the row s[0, len), len >= 1, and its value
// ---------------------------------------------------------------------------

// [+-]?[0-9]+ with the value in [lo, hi]
struct IntOp {
  using Out = int64_t;
  static constexpr bool kEmptyIsNull = true;
  int64_t lo, hi;
  DEV_INLINE uint8_t parse(const uint8_t* s, int64_t len, int64_t* out) const {
    bool neg = s[0] == '-';
    int64_t i = (neg || s[0] == '+') ? 1 : 0;
    if (i == len) return kHost;
    // |value| <= 2^63 - 1, or 2^63 for a negative one
    const uint64_t top = 922337203685477580ull, last = neg ? 8 : 7;
    uint64_t acc = 0;
    for (; i < len; ++i) {
      uint8_t d = s[i] - '0';
      if (d > 9) return kHost;
      if (acc > top || (acc == top && d > last)) return kHost;
      acc = acc * 10 + d;
    }
    int64_t v = (int64_t)(neg ? 0 - acc : acc);
    if (v < lo || v > hi) return kHost;
    *out = v;
    return kParsed;
  }
};

// [+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+) as an integer scaled by 10^scale; digits
// past `scale` must be 0 (the host rounds the others), |value| <= max_abs
struct DecimalOp {
  using Out = int64_t;
  static constexpr bool kEmptyIsNull = true;
  int scale;
  uint64_t max_abs;  // < 10^18, so acc * 10 + 9 below cannot wrap
  DEV_INLINE uint8_t parse(const uint8_t* s, int64_t len, int64_t* out) const {
    bool neg = s[0] == '-';
    int64_t i = (neg || s[0] == '+') ? 1 : 0;
    uint64_t acc = 0;
    bool digits = false;
    for (; i < len && is_digit(s[i]); ++i) {
      acc = acc * 10 + (s[i] - '0');
      if (acc > max_abs) return kHost;
      digits = true;
    }
    int frac = 0;
    if (i < len && s[i] == '.') {
      for (++i; i < len && is_digit(s[i]); ++i) {
        digits = true;
        if (frac < scale) {
          acc = acc * 10 + (s[i] - '0');
          if (acc > max_abs) return kHost;
          ++frac;
        } else if (s[i] != '0') {
          return kHost;
        }
      }
    }
    if (i < len || !digits) return kHost;
    for (; frac < scale; ++frac) {
      acc *= 10;
      if (acc > max_abs) return kHost;
    }
    *out = neg ? -(int64_t)acc : (int64_t)acc;
    return kParsed;
  }
};

// exact powers of ten in a double: 10^0 .. 10^22
__device__ const double kPow10[23] = {
    1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
    1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

constexpr int kPow5Min = -342, kPow5Max = 308;

// [+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)? to the nearest double:
// w * 10^q with w the significant digits (at most 19, so w < 2^64).
struct FloatOp {
  using Out = double;
  static constexpr bool kEmptyIsNull = true;
  const uint64_t* pow5;  // [651][2]: {low, high} 64 bits of 5^q, q >= -342

  DEV_INLINE uint8_t parse(const uint8_t* s, int64_t len, double* out) const {
    bool neg = s[0] == '-';
    int64_t i = (neg || s[0] == '+') ? 1 : 0;
    uint64_t w = 0;
    int sig = 0;        // significant digits in w
    int64_t q = 0;      // decimal exponent of w's last digit
    bool digits = false;
    for (; i < len && is_digit(s[i]); ++i) {
      digits = true;
      if (sig == 0 && s[i] == '0') continue;   // leading zero
      if (++sig > 19) return kHost;
      w = w * 10 + (s[i] - '0');
    }
    if (i < len && s[i] == '.') {
      for (++i; i < len && is_digit(s[i]); ++i) {
        digits = true;
        --q;
        if (sig == 0 && s[i] == '0') continue;
        if (++sig > 19) return kHost;
        w = w * 10 + (s[i] - '0');
      }
    }
    if (!digits) return kHost;
    if (i < len) {
      if (s[i] != 'e' && s[i] != 'E') return kHost;
      ++i;
      bool eneg = i < len && s[i] == '-';
      if (i < len && (eneg || s[i] == '+')) ++i;
      if (i == len) return kHost;
      int64_t e = 0;
      for (; i < len; ++i) {
        if (!is_digit(s[i])) return kHost;
        if (e < 100000) e = e * 10 + (s[i] - '0');   // saturate: far outside
      }
      q += eneg ? -e : e;
    }
    if (w == 0) {
      *out = neg ? -0.0 : 0.0;
      return kParsed;
    }
    // Clinger: w and 10^|q| are both exact, so one IEEE operation rounds once
    if (w <= (1ull << 53) && q >= -22 && q <= 22) {
      double d = (double)w;
      d = q < 0 ? d / kPow10[-q] : d * kPow10[q];
      *out = neg ? -d : d;
      return kParsed;
    }
    if (q < kPow5Min || q > kPow5Max) return kHost;  // subnormal, 0 or inf
    // Eisel-Lemire: w, shifted to 64 significant bits, times the 128-bit
    // 5^q.  The upper 64 bits of the product hold the 54-bit result unless
    // the bits below could still carry into it.
    int lz = __clzll((long long)w);
    w <<= lz;
    const uint64_t* p = pow5 + 2 * (q - kPow5Min);
    uint64_t p_lo = p[0], p_hi = p[1];
    // floor(q * log2(10)) + 64 + 1023 - lz
    int64_t e2 = ((217706 * q) >> 16) + 64 + 1023 - lz;
    uint64_t x_hi = __umul64hi(w, p_hi), x_lo = w * p_hi;
    if ((x_hi & 0x1FF) == 0x1FF && x_lo + w < x_lo) {
      // the truncated low half of 5^q could matter: add its product in
      uint64_t y_hi = __umul64hi(w, p_lo), y_lo = w * p_lo;
      uint64_t m_lo = x_lo + y_hi, m_hi = x_hi + (m_lo < x_lo ? 1 : 0);
      if ((m_hi & 0x1FF) == 0x1FF && m_lo + 1 == 0 && y_lo + w < y_lo)
        return kHost;                                // still cannot decide
      x_hi = m_hi;
      x_lo = m_lo;
    }
    int msb = (int)(x_hi >> 63);
    uint64_t m = x_hi >> (msb + 9);                  // 54 bits
    e2 -= 1 ^ msb;
    // exactly half way between two doubles, as far as the product shows
    if (x_lo == 0 && (x_hi & 0x1FF) == 0 && (m & 3) == 1) return kHost;
    m += m & 1;
    m >>= 1;
    if (m >> 53) {
      m >>= 1;
      ++e2;
    }
    if (e2 <= 0 || e2 >= 0x7FF) return kHost;        // subnormal or infinite
    uint64_t bits = ((uint64_t)e2 << 52) | (m & 0x000FFFFFFFFFFFFFull) |
                    (neg ? 0x8000000000000000ull : 0);
    *out = __longlong_as_double((long long)bits);
    return kParsed;
  }
};

// days since 1970-01-01 of a proleptic Gregorian date (Hinnant)
DEV_INLINE int64_t days_from_civil(int y, int m, int d) {
  y -= m <= 2;
  int era = (y >= 0 ? y : y - 399) / 400;
  int yoe = y - era * 400;
  int doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5 + d - 1;
  int doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return (int64_t)era * 146097 + doe - 719468;
}

// two digits at s[i], or -1
DEV_INLINE int two_digits(const uint8_t* s, int i) {
  if (!is_digit(s[i]) || !is_digit(s[i + 1])) return -1;
  return (s[i] - '0') * 10 + (s[i + 1] - '0');
}

// YYYY-MM-DD (sep == 0) as days, YYYY-MM-DD<sep>HH:MM:SS as microseconds
template <typename T>
struct DateTimeOp {
  using Out = T;
  static constexpr bool kEmptyIsNull = false;  // the host raises on ""
  uint8_t sep;
  DEV_INLINE uint8_t parse(const uint8_t* s, int64_t len, T* out) const {
    if (len != (sep ? 19 : 10)) return kHost;
    int yh = two_digits(s, 0), yl = two_digits(s, 2);
    int mo = two_digits(s, 5), d = two_digits(s, 8);
    if (yh < 0 || yl < 0 || mo < 0 || d < 0 || s[4] != '-' || s[7] != '-')
      return kHost;
    int y = yh * 100 + yl;
    if (y < 1 || mo < 1 || mo > 12 || d < 1) return kHost;
    bool leap = (y % 4 == 0 && y % 100 != 0) || y % 400 == 0;
    int dim = mo == 2 ? (leap ? 29 : 28)
                      : ((mo == 4 || mo == 6 || mo == 9 || mo == 11) ? 30 : 31);
    if (d > dim) return kHost;
    int64_t v = days_from_civil(y, mo, d);
    if (sep) {
      int h = two_digits(s, 11), mi = two_digits(s, 14);
      int sec = two_digits(s, 17);
      if (s[10] != sep || s[13] != ':' || s[16] != ':' || h < 0 || h > 23 ||
          mi < 0 || mi > 59 || sec < 0 || sec > 59)
        return kHost;
      v = (v * 86400 + h * 3600 + mi * 60 + sec) * 1000000;
    }
    *out = (T)v;
    return kParsed;
  }
};

// ---------------------------------------------------------------------------
// the driver: stage 256 rows' bytes in LDS, or read them in place
// ---------------------------------------------------------------------------
template <typename Op>
DEV_INLINE void parse_row(const Op& op, const uint8_t* s, int64_t len,
                          bool is_valid, typename Op::Out* value,
                          uint8_t* status) {
  typename Op::Out v = 0;
  uint8_t st = kNull;
  if (is_valid && (len > 0 || !Op::kEmptyIsNull)) {
    st = len > 0 ? op.parse(s, len, &v) : (uint8_t)kHost;
    if (st != kParsed) v = 0;
  }
  *value = v;
  *status = st;
}

template <typename Op>
__global__ void __launch_bounds__(kParseBlock)
parse_kernel(const int64_t* offs, const uint8_t* bytes, int64_t nbytes,
             const bool* valid, int64_t n, bool staged, Op op,
             typename Op::Out* values, uint8_t* status) {
  __shared__ uint4 tile4[kParseTile / 16];
  uint8_t* tile = (uint8_t*)tile4;
  int64_t tiles = (n + kParseBlock - 1) / kParseBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    int64_t r0 = t * kParseBlock;
    int64_t r1 = r0 + kParseBlock < n ? r0 + kParseBlock : n;
    int64_t lo = offs[r0], hi = offs[r1];  // the same in every thread
    // bytes[lo] lands at tile[mis]: 16-byte chunks of the tile are then
    // 16-byte aligned in global memory too
    int mis = (int)((uintptr_t)(bytes + lo) & 15);
    bool fits = staged && lo >= 0 && lo <= hi && hi <= nbytes &&
                hi - lo + mis <= kParseTile;
    if (fits) {
      int end = mis + (int)(hi - lo);
      const uint8_t* g = bytes + lo - mis;            // tile[k] = g[k]
      for (int c = threadIdx.x * 16; c < end; c += kParseBlock * 16) {
        if (c >= mis && c + 16 <= end) {
          tile4[c / 16] = *(const uint4*)(g + c);
        } else {                                      // clipped head or tail
          int k0 = c > mis ? c : mis, k1 = c + 16 < end ? c + 16 : end;
          for (int k = k0; k < k1; ++k) tile[k] = g[k];
        }
      }
      __syncthreads();
    }
    int64_t row = r0 + threadIdx.x;
    if (row < r1) {
      int64_t a = offs[row], b = offs[row + 1];
      bool ok = !valid || valid[row];
      if (fits) {
        // offsets that leave the span are not followed
        if (a < lo || a > b || b > hi) {
          values[row] = 0;
          status[row] = ok ? kHost : kNull;
        } else {
          parse_row(op, tile + mis + (a - lo), b - a, ok, values + row,
                    status + row);
        }
      } else if (a < 0 || a > b || b > nbytes) {
        values[row] = 0;
        status[row] = ok ? kHost : kNull;
      } else {
        parse_row(op, bytes + a, b - a, ok, values + row, status + row);
      }
    }
    __syncthreads();  // the tile is refilled by the next round
  }
}

template <typename Op>
static std::vector<Tensor> run_parse(const StrCol& c, const bool* vptr,
                                     const Op& op, torch::ScalarType out_type,
                                     const torch::Device& dev) {
  auto values = torch::empty({c.n}, torch::dtype(out_type).device(dev));
  auto status = torch::empty({c.n}, torch::dtype(torch::kUInt8).device(dev));
  if (c.n > 0)
    hipLaunchKernelGGL(parse_kernel<Op>, dim3(grid_1d(c.n, kParseBlock)),
                       dim3(kParseBlock), 0, cur_stream(), c.offs, c.bytes,
                       c.nbytes, vptr, c.n, g_staged, op,
                       (typename Op::Out*)values.data_ptr(),
                       status.data_ptr<uint8_t>());
  return {values, status};
}

bool strparse_staging(bool on) {
  bool was = g_staged;
  g_staged = on;
  return was;
}

std::vector<Tensor> str_parse_int(Tensor offsets, Tensor bytes, OptTensor valid,
                                  int64_t lo, int64_t hi) {
  StrCol c = check_strcol("str_parse_int", offsets, bytes);
  const bool* vptr = check_valid("str_parse_int", valid, c.n, offsets.device());
  TORCH_CHECK(lo <= hi, "str_parse_int: lo must be <= hi, got ", lo, " > ", hi);
  return run_parse(c, vptr, IntOp{lo, hi}, torch::kInt64, offsets.device());
}

std::vector<Tensor> str_parse_decimal(Tensor offsets, Tensor bytes,
                                      OptTensor valid, int64_t scale,
                                      int64_t max_abs) {
  StrCol c = check_strcol("str_parse_decimal", offsets, bytes);
  const bool* vptr =
      check_valid("str_parse_decimal", valid, c.n, offsets.device());
  TORCH_CHECK(scale >= 0 && scale <= 18,
              "str_parse_decimal: scale must be in [0, 18], got ", scale);
  TORCH_CHECK(max_abs >= 0 && max_abs < 1000000000000000000ll,
              "str_parse_decimal: max_abs must be in [0, 10^18), got ",
              max_abs);
  return run_parse(c, vptr, DecimalOp{(int)scale, (uint64_t)max_abs},
                   torch::kInt64, offsets.device());
}

std::vector<Tensor> str_parse_float(Tensor offsets, Tensor bytes,
                                    OptTensor valid, Tensor pow5) {
  StrCol c = check_strcol("str_parse_float", offsets, bytes);
  auto dev = offsets.device();
  const bool* vptr = check_valid("str_parse_float", valid, c.n, dev);
  check_tensor("str_parse_float", "pow5", pow5, torch::kInt64, dev);
  TORCH_CHECK(pow5.dim() == 2 && pow5.size(0) == kPow5Max - kPow5Min + 1 &&
                  pow5.size(1) == 2,
              "str_parse_float: pow5 must be int64 [651, 2]");
  return run_parse(c, vptr, FloatOp{(const uint64_t*)pow5.data_ptr<int64_t>()},
                   torch::kFloat64, dev);
}

std::vector<Tensor> str_parse_datetime(Tensor offsets, Tensor bytes,
                                       OptTensor valid, int64_t sep) {
  StrCol c = check_strcol("str_parse_datetime", offsets, bytes);
  auto dev = offsets.device();
  const bool* vptr = check_valid("str_parse_datetime", valid, c.n, dev);
  TORCH_CHECK(sep == 0 || sep == ' ' || sep == 'T',
              "str_parse_datetime: sep must be 0, ' ' or 'T', got ", sep);
  if (sep == 0)
    return run_parse(c, vptr, DateTimeOp<int32_t>{0}, torch::kInt32, dev);
  return run_parse(c, vptr, DateTimeOp<int64_t>{(uint8_t)sep}, torch::kInt64,
                   dev);
}

// ---------------------------------------------------------------------------
// formatting: a length kernel, offsets_from_lens, a write kernel; one thread
// per row, null rows are empty
// ---------------------------------------------------------------------------
struct IntFmt {
  using In = int64_t;
  DEV_INLINE static int length(int64_t v) {
    uint64_t a = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    int k = v < 0 ? 2 : 1;
    for (; a >= 10; a /= 10) ++k;
    return k;
  }
  // writes the row that ends before `end`
  DEV_INLINE static void write(int64_t v, uint8_t* end) {
    uint64_t a = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    do {
      *--end = '0' + (uint8_t)(a % 10);
      a /= 10;
    } while (a);
    if (v < 0) *--end = '-';
  }
};

// days in years 0001-9999 only (the caller checks): YYYY-MM-DD
struct DateFmt {
  using In = int32_t;
  DEV_INLINE static int length(int32_t) { return 10; }
  DEV_INLINE static void write(int32_t days, uint8_t* end) {
    int z = days + 719468;                      // > 0 for year >= 1 (Hinnant)
    int era = z / 146097, doe = z - era * 146097;
    int yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    int doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    int mp = (5 * doy + 2) / 153;
    int d = doy - (153 * mp + 2) / 5 + 1;
    int m = mp < 10 ? mp + 3 : mp - 9;
    int y = yoe + era * 400 + (m <= 2);
    uint8_t* o = end - 10;
    o[0] = '0' + y / 1000;
    o[1] = '0' + y / 100 % 10;
    o[2] = '0' + y / 10 % 10;
    o[3] = '0' + y % 10;
    o[4] = '-';
    o[5] = '0' + m / 10;
    o[6] = '0' + m % 10;
    o[7] = '-';
    o[8] = '0' + d / 10;
    o[9] = '0' + d % 10;
  }
};

template <typename Fmt>
__global__ void format_len_kernel(const typename Fmt::In* values,
                                  const bool* valid, int64_t n,
                                  int64_t* lens) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    lens[i] = (valid && !valid[i]) ? 0 : Fmt::length(values[i]);
}

template <typename Fmt>
__global__ void format_write_kernel(const typename Fmt::In* values, int64_t n,
                                    const int64_t* out_off, uint8_t* out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t end = out_off[i + 1];
    if (end > out_off[i]) Fmt::write(values[i], out + end);
  }
}

template <typename Fmt>
static std::vector<Tensor> run_format(const char* who, const Tensor& values,
                                      const OptTensor& valid,
                                      torch::ScalarType in_type) {
  TORCH_CHECK(values.is_cuda(), who, ": values must be on a GPU device");
  auto dev = values.device();
  check_tensor(who, "values", values, in_type, dev);
  TORCH_CHECK(values.dim() == 1, who, ": values must have one dimension");
  int64_t n = values.numel();
  const bool* vptr = check_valid(who, valid, n, dev);
  auto in = (const typename Fmt::In*)values.data_ptr();
  auto lens = torch::empty({n}, torch::dtype(torch::kInt64).device(dev));
  int block = 256, grid = grid_1d(n, block);
  if (n > 0)
    hipLaunchKernelGGL(format_len_kernel<Fmt>, dim3(grid), dim3(block), 0,
                       cur_stream(), in, vptr, n, lens.data_ptr<int64_t>());
  auto [out_off, total] = offsets_from_lens(lens);
  auto out = torch::empty({total}, torch::dtype(torch::kUInt8).device(dev));
  if (total > 0)
    hipLaunchKernelGGL(format_write_kernel<Fmt>, dim3(grid), dim3(block), 0,
                       cur_stream(), in, n, out_off.data_ptr<int64_t>(),
                       out.data_ptr<uint8_t>());
  return {out_off, out};
}

std::vector<Tensor> format_int(Tensor values, OptTensor valid) {
  return run_format<IntFmt>("format_int", values, valid, torch::kInt64);
}

std::vector<Tensor> format_date(Tensor days, OptTensor valid) {
  return run_format<DateFmt>("format_date", days, valid, torch::kInt32);
}
