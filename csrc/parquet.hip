// Parquet page decode in device memory (gfx950, wave64): raw Snappy blocks,
// the RLE / bit-packed hybrid of levels, dictionary indices and booleans,
// PLAIN fixed-width values, and the PLAIN BYTE_ARRAY dictionary page of a
// string column.  The host (kernels/parquet.py) walks the page headers and
// uploads one row group's column-chunk bytes and one descriptor table; every
// kernel here reads its pages from that table.
//
// One buffer `buf` holds the uploaded bytes and, behind them, the arena the
// Snappy kernel decompresses into, so a page's payload is a range of `buf`
// whether or not it was compressed.  A descriptor row is kPqDesc int64:
//
//   [0] src_off  [1] src_len   compressed bytes (src_len 0: nothing to do)
//   [2] dst_off  [3] dst_len   where they decompress to, and the size the
//                              page header promises
//   [4] lvl_off  [5] lvl_len   definition levels.  lvl_len -1: a V1 page,
//                              whose payload [lvl_off, val_end) begins with a
//                              4-byte length, the levels, then the values
//   [6] val_off  [7] val_end   values (V1 with levels: found as above)
//   [8] num_values  [9] first_row   rows [first_row, first_row + num_values)
//   [10] encoding   0 PLAIN, 1 dictionary indices, 2 RLE booleans
//
// Every kernel checks its row against the size of `buf` and of its outputs
// before it touches memory, and every read and write of page content is
// checked against the page's own range; what fails sets a bit of status[page]
// (kPqBadDesc, kPqCorrupt) and leaves the rest of the page unwritten.  The
// host reads the status once per row group and hands a flagged chunk to
// pyarrow.
//
//   snappy    one wave per page.  The element stream is serial, so lane 0
//             parses it, but from LDS: the wave stages 1024 compressed bytes
//             with one 16-byte load per lane, lane 0 turns up to 64 elements
//             into (src, dst, len) records in LDS, then the 64 lanes move the
//             bytes of each record: a literal 8 bytes per lane and step, a
//             copy (at most 64 bytes) one byte per lane from
//             out[dst - offset + lane % offset], which is the repeating
//             pattern an overlapping copy (offset < len) stands for and reads
//             only bytes that earlier records wrote.  A copy's source may
//             have been stored by this wave a moment earlier.  The trailing
//             window is not kept in LDS (offsets reach 64 KiB and beyond, and
//             that much LDS per wave would leave one wave per CU); the copy
//             goes through global memory, where one wave's vector memory
//             operations reach the CU's L1 in program order, and a
//             wavefront-scope fence after each record keeps the compiler from
//             moving a load over the store it depends on.
//   levels    one wave per page, bit width 1.  Lane 0 walks up to 64 run
//             headers (a serial chain of varints) into LDS; the wave expands
//             them 64 values at a time, RLE runs as broadcasts, bit-packed
//             runs from an unaligned 64-bit window at bit k * bw.  A ballot
//             of the valid lanes ranks each valid row among the valid rows of
//             its page, which gives map[first_row + rank] = row: the row the
//             page's rank-th stored value belongs to.  Writes validity, map
//             and the page's count of stored values.
//   plain     blocks of 256 threads, (page, slice of the page) per block.
//             Payloads start at any byte, so values are loaded unaligned; an
//             integer of 4, 8 or (FIXED_LEN_BYTE_ARRAY, big-endian) 1..8
//             bytes is sign-extended and its low `out_width` bytes stored;
//             booleans are unpacked from bits.  Value j of the page goes to
//             row map[first_row + j], or first_row + j without nulls.
//   rle       one wave per page, the hybrid above at the bit width in the
//             values' first byte (booleans: width 1 behind a 4-byte length).
//             The index is checked against the dictionary's size and the
//             gather out[row] = dict[idx] is fused in; without a dictionary
//             tensor the index itself is stored (string codes, booleans).
//   strings   one wave on a string column's dictionary page: 1024 bytes
//             staged as in snappy, lane 0 walks the 4-byte lengths of up to
//             64 values into LDS and writes their offsets, the lanes copy the
//             bytes (a value per lane; from 64 bytes on, the whole wave).
#include "common.h"
#include "host_args.h"
#include "api.h"

constexpr int kPqDesc = 12;
constexpr int kPqStage = 1024;   // bytes staged per step: one uint4 per lane
constexpr int kPqPlainBlock = 256;
constexpr int64_t kPqMaxPage = (int64_t)1 << 30;

enum : int32_t { kPqBadDesc = 1, kPqCorrupt = 2 };
enum { kEncPlain = 0, kEncDict = 1, kEncRleBool = 2 };

// ---------------------------------------------------------------------------
// a page's ranges, checked
// ---------------------------------------------------------------------------
struct PqPage {
  int64_t lvl_beg, lvl_end, val_beg, val_end, nv, first_row;
  int enc;
  int32_t err;
};

DEV_INLINE uint32_t le32(const uint8_t* p) {
  return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) |
         ((uint32_t)p[3] << 24);
}

DEV_INLINE PqPage load_page(const uint8_t* buf, int64_t buf_n,
                            const int64_t* d, int64_t nrows) {
  PqPage pg;
  const int64_t lvl_off = d[4], lvl_len = d[5], val_off = d[6];
  pg.val_end = d[7];
  pg.nv = d[8];
  pg.first_row = d[9];
  pg.enc = (int)d[10];
  pg.err = 0;
  pg.lvl_beg = pg.lvl_end = 0;
  pg.val_beg = val_off;
  if (pg.nv < 0 || pg.nv >= kPqMaxPage || pg.first_row < 0 ||
      pg.first_row + pg.nv > nrows || val_off < 0 || val_off > pg.val_end ||
      pg.val_end > buf_n || pg.val_end - val_off >= kPqMaxPage ||
      lvl_off < 0 || lvl_off > buf_n) {
    pg.err = kPqBadDesc;
    return pg;
  }
  if (lvl_len == -1) {
    if (lvl_off != val_off || pg.val_end - lvl_off < 4) {
      pg.err = lvl_off != val_off ? kPqBadDesc : kPqCorrupt;
      return pg;
    }
    const int64_t len = le32(buf + lvl_off);
    pg.lvl_beg = lvl_off + 4;
    pg.lvl_end = pg.lvl_beg + len;
    if (pg.lvl_end > pg.val_end) {
      pg.err = kPqCorrupt;
      return pg;
    }
    pg.val_beg = pg.lvl_end;
  } else {
    if (lvl_len < 0 || lvl_len >= kPqMaxPage || lvl_off + lvl_len > buf_n) {
      pg.err = kPqBadDesc;
      return pg;
    }
    pg.lvl_beg = lvl_off;
    pg.lvl_end = lvl_off + lvl_len;
  }
  return pg;
}

// buf[a, a + 16) for the 16-byte aligned a = (abs & ~15) + 16 * lane into
// win: kPqStage bytes that hold buf[abs] at index abs & 15.  `buf` is 16-byte
// aligned; bytes from buf_n on read as zero.
DEV_INLINE void stage_window(const uint8_t* buf, int64_t buf_n, int64_t abs,
                             uint8_t* win, int lane) {
  const int64_t a = (abs & ~(int64_t)15) + 16 * lane;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (a + 16 <= buf_n) {
    v = *(const uint4*)(buf + a);
  } else {
    uint32_t w[4] = {0, 0, 0, 0};
    for (int i = 0; i < 16 && a + i < buf_n; ++i)
      w[i >> 2] |= (uint32_t)buf[a + i] << (8 * (i & 3));
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  ((uint4*)win)[lane] = v;
}

// ---------------------------------------------------------------------------
// Snappy
// ---------------------------------------------------------------------------
constexpr uint32_t kLiteral = 0x80000000u;

__global__ void __launch_bounds__(WAVE)
pq_snappy_kernel(uint8_t* buf, int64_t buf_n, const int64_t* desc,
                 int32_t* status) {
  __shared__ __attribute__((aligned(16))) uint8_t win[kPqStage];
  __shared__ uint32_t r_src[WAVE], r_dst[WAVE], r_len[WAVE];
  __shared__ uint32_t ctl[4];  // records, ip, op, error
  const int lane = threadIdx.x;
  const int64_t* d = desc + (int64_t)blockIdx.x * kPqDesc;
  const int64_t src_off = d[0], in_len = d[1], dst_off = d[2], out_len = d[3];
  if (in_len == 0) return;
  if (src_off < 0 || in_len < 0 || in_len >= kPqMaxPage ||
      src_off + in_len > buf_n || dst_off < 0 || out_len < 0 ||
      out_len >= kPqMaxPage || dst_off + out_len > buf_n) {
    if (lane == 0) atomicOr(&status[blockIdx.x], kPqBadDesc);
    return;
  }
  const uint8_t* in = buf + src_off;
  uint8_t* out = buf + dst_off;
  const uint32_t n_in = (uint32_t)in_len, n_out = (uint32_t)out_len;

  // the preamble: every lane reads the same few bytes
  uint32_t ip = 0, op = 0, shift = 0;
  uint64_t promised = 0;
  bool err = true;
  while (ip < n_in && shift <= 28) {
    const uint32_t b = in[ip++];
    promised |= (uint64_t)(b & 0x7F) << shift;
    if (!(b & 0x80)) {
      err = false;
      break;
    }
    shift += 7;
  }
  err = err || promised != (uint64_t)out_len;

  while (!err && ip < n_in) {
    const int64_t abs = src_off + ip;
    stage_window(buf, buf_n, abs, win, lane);
    __syncthreads();
    if (lane == 0) {
      const uint32_t w0 = (uint32_t)(abs & 15);
      uint32_t c = 0, q = ip, o = op, e = 0;
      while (c < WAVE && q < n_in) {
        const uint32_t wi = w0 + (q - ip);
        // a tag and the (at most 4) bytes behind it must be staged; the
        // first element of a window always is, since w0 <= 15
        if (wi + 5 > kPqStage) break;
        const uint32_t tag = win[wi];
        if ((tag & 3) == 0) {
          uint32_t l = tag >> 2, hdr = 1;
          if (l >= 60) {
            const uint32_t nb = l - 59;
            if ((uint64_t)q + 1 + nb > n_in) { e = 1; break; }
            l = 0;
            for (uint32_t k = 0; k < nb; ++k)
              l |= (uint32_t)win[wi + 1 + k] << (8 * k);
            hdr = 1 + nb;
          }
          const uint64_t len = (uint64_t)l + 1;
          if ((uint64_t)q + hdr + len > n_in || (uint64_t)o + len > n_out) {
            e = 1;
            break;
          }
          r_src[c] = q + hdr;
          r_dst[c] = o;
          r_len[c] = (uint32_t)len | kLiteral;
          q += hdr + (uint32_t)len;
          o += (uint32_t)len;
        } else {
          const uint32_t kind = tag & 3;
          const uint32_t hdr = kind == 1 ? 2 : kind == 2 ? 3 : 5;
          if ((uint64_t)q + hdr > n_in) { e = 1; break; }
          uint32_t len, off;
          if (kind == 1) {
            len = 4 + ((tag >> 2) & 7);
            off = ((tag >> 5) << 8) | win[wi + 1];
          } else {
            len = 1 + (tag >> 2);
            off = win[wi + 1] | ((uint32_t)win[wi + 2] << 8);
            if (kind == 3)
              off |= ((uint32_t)win[wi + 3] << 16) |
                     ((uint32_t)win[wi + 4] << 24);
          }
          if (off == 0 || off > o || (uint64_t)o + len > n_out) {
            e = 1;
            break;
          }
          r_src[c] = off;
          r_dst[c] = o;
          r_len[c] = len;
          q += hdr;
          o += len;
        }
        ++c;
      }
      ctl[0] = c;
      ctl[1] = q;
      ctl[2] = o;
      ctl[3] = e;
    }
    __syncthreads();
    const uint32_t cnt = ctl[0];
    for (uint32_t r = 0; r < cnt; ++r) {
      const uint32_t len = r_len[r], s = r_src[r], dst = r_dst[r];
      if (len & kLiteral) {
        const uint32_t n = len & ~kLiteral;
        const uint8_t* sp = in + s;
        uint8_t* dp = out + dst;
        for (uint32_t i = lane * 8; i + 8 <= n; i += WAVE * 8) {
          uint64_t w;
          __builtin_memcpy(&w, sp + i, 8);
          __builtin_memcpy(dp + i, &w, 8);
        }
        const uint32_t i = (n & ~7u) + lane;
        if (i < n) dp[i] = sp[i];
      } else if ((uint32_t)lane < len) {
        // len <= 64: one byte per lane; sources lie before dst
        const uint32_t k = s >= len ? lane : lane % s;
        const uint8_t b = out[dst - s + k];
        out[dst + lane] = b;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    ip = ctl[1];
    op = ctl[2];
    err = ctl[3] != 0;
    __syncthreads();
  }
  if (!err && op != n_out) err = true;
  if (err && lane == 0) atomicOr(&status[blockIdx.x], kPqCorrupt);
}

// ---------------------------------------------------------------------------
// RLE / bit-packed hybrid, one wave per page
// ---------------------------------------------------------------------------
struct RleRuns {
  uint32_t hdr[WAVE];  // values of the run << 1 | 1 when bit-packed
  uint32_t pay[WAVE];  // the RLE value, or where the packed bits start
  uint32_t ctl[3];     // runs, position, error
};

// bits [8 * byte, 8 * byte + 64) of p[0, len), zeros past the end
DEV_INLINE uint64_t bit_window(const uint8_t* p, int64_t byte, int64_t len) {
  uint64_t w = 0;
  if (byte + 8 <= len) {
    __builtin_memcpy(&w, p + byte, 8);
  } else {
    for (int i = 0; i < 8 && byte + i < len; ++i)
      w |= (uint64_t)p[byte + i] << (8 * i);
  }
  return w;
}

// Decodes nv values of width bw from the runs in p[0, len) and calls
// f(i, value, active) for i in [0, nv), 64 consecutive i per call, every
// lane of the wave taking part (active false past a run's end).  Returns
// false when the runs are malformed or end early; bw 0 needs no runs.
template <class F>
DEV_INLINE bool rle_hybrid(const uint8_t* p, int64_t len, int bw, int64_t nv,
                           RleRuns& s, int lane, F&& f) {
  const uint32_t mask = bw >= 32 ? 0xFFFFFFFFu : ((1u << bw) - 1);
  const int64_t n = len;
  int64_t out_i = 0;
  uint32_t pos = 0;
  while (out_i < nv) {
    if (lane == 0) {
      uint32_t c = 0, e = 0;
      int64_t q = pos, done = out_i;
      while (c < WAVE && done < nv && q < n) {
        uint32_t h = 0, shift = 0;
        bool ended = false;
        while (q < n && shift <= 28) {
          const uint32_t b = p[q++];
          h |= (b & 0x7F) << shift;
          if (!(b & 0x80)) {
            ended = true;
            break;
          }
          shift += 7;
        }
        if (!ended) { e = 1; break; }
        int64_t take;
        uint32_t pay;
        if (h & 1) {
          // groups of 8 values; the last group is padded, clamp to nv
          const int64_t groups = h >> 1;
          take = groups * 8 < nv - done ? groups * 8 : nv - done;
          if ((take * bw + 7) / 8 > n - q) { e = 1; break; }
          pay = (uint32_t)q;
          q = groups * bw < n - q ? q + groups * bw : n;
        } else {
          const int vb = (bw + 7) / 8;
          if (vb > n - q) { e = 1; break; }
          pay = 0;
          for (int k = 0; k < vb; ++k) pay |= (uint32_t)p[q + k] << (8 * k);
          q += vb;
          take = (int64_t)(h >> 1) < nv - done ? (h >> 1) : nv - done;
        }
        if (take > 0) {
          s.hdr[c] = ((uint32_t)take << 1) | (h & 1);
          s.pay[c] = pay;
          ++c;
          done += take;
        }
      }
      if (c == 0 && !e) {
        if (bw == 0) {
          s.hdr[0] = (uint32_t)(nv - done) << 1;
          s.pay[0] = 0;
          c = 1;
        } else {
          e = 1;  // the runs end before the page's values do
        }
      }
      s.ctl[0] = c;
      s.ctl[1] = (uint32_t)q;
      s.ctl[2] = e;
    }
    __syncthreads();
    const uint32_t cnt = s.ctl[0];
    const bool bad = s.ctl[2] != 0;
    pos = s.ctl[1];
    for (uint32_t r = 0; r < cnt; ++r) {
      const uint32_t h = s.hdr[r], pay = s.pay[r];
      const int64_t run = h >> 1;
      for (int64_t k0 = 0; k0 < run; k0 += WAVE) {
        const int64_t k = k0 + lane;
        const bool active = k < run;
        uint32_t v = pay;
        if (h & 1) {
          v = 0;
          if (active) {
            const int64_t bit = k * bw;
            v = (uint32_t)(bit_window(p, pay + (bit >> 3), n) >> (bit & 7)) &
                mask;
          }
        }
        f(out_i + k, v & mask, active);
      }
      out_i += run;
    }
    __syncthreads();
    if (bad) return false;
  }
  return true;
}

__global__ void __launch_bounds__(WAVE)
pq_levels_kernel(const uint8_t* buf, int64_t buf_n, const int64_t* desc,
                 int64_t nrows, bool* validity, int32_t* map, int32_t* stored,
                 int32_t* status) {
  __shared__ RleRuns runs;
  const int lane = threadIdx.x;
  const PqPage pg =
      load_page(buf, buf_n, desc + (int64_t)blockIdx.x * kPqDesc, nrows);
  if (pg.err) {
    if (lane == 0) {
      atomicOr(&status[blockIdx.x], pg.err);
      stored[blockIdx.x] = 0;
    }
    return;
  }
  int32_t base = 0;
  const bool ok = rle_hybrid(
      buf + pg.lvl_beg, pg.lvl_end - pg.lvl_beg, 1, pg.nv, runs, lane,
      [&](int64_t i, uint32_t v, bool active) {
        const bool valid = active && v == 1;
        const uint64_t m = __ballot(valid);
        if (active) {
          const int64_t row = pg.first_row + i;
          validity[row] = valid;
          if (valid) {
            const int rank = __popcll(m & (((uint64_t)1 << lane) - 1));
            map[pg.first_row + base + rank] = (int32_t)row;
          }
        }
        base += __popcll(m);
      });
  if (lane == 0) {
    stored[blockIdx.x] = ok ? base : 0;
    if (!ok) atomicOr(&status[blockIdx.x], kPqCorrupt);
  }
}

// ---------------------------------------------------------------------------
// values
// ---------------------------------------------------------------------------
DEV_INLINE void store_low(uint8_t* out, int64_t row, int width, uint64_t v) {
  if (width == 8) ((uint64_t*)out)[row] = v;
  else if (width == 4) ((uint32_t*)out)[row] = (uint32_t)v;
  else if (width == 2) ((uint16_t*)out)[row] = (uint16_t)v;
  else out[row] = (uint8_t)v;
}

// in_width 0: booleans, one bit each; big_endian: FIXED_LEN_BYTE_ARRAY
__global__ void __launch_bounds__(kPqPlainBlock)
pq_plain_kernel(const uint8_t* buf, int64_t buf_n, const int64_t* desc,
                int64_t nrows, const int32_t* map, const int32_t* stored,
                uint8_t* out, int in_width, bool big_endian, int out_width,
                int32_t* status) {
  const PqPage pg =
      load_page(buf, buf_n, desc + (int64_t)blockIdx.x * kPqDesc, nrows);
  if (pg.enc != kEncPlain) return;
  if (pg.err) {
    if (threadIdx.x == 0) atomicOr(&status[blockIdx.x], pg.err);
    return;
  }
  int64_t n = stored ? stored[blockIdx.x] : pg.nv;
  if (n > pg.nv) n = pg.nv;
  const int64_t need = in_width ? n * in_width : (n + 7) / 8;
  if (need > pg.val_end - pg.val_beg) {
    if (threadIdx.x == 0) atomicOr(&status[blockIdx.x], kPqCorrupt);
    return;
  }
  const uint8_t* p = buf + pg.val_beg;
  for (int64_t j = (int64_t)blockIdx.y * kPqPlainBlock + threadIdx.x; j < n;
       j += (int64_t)gridDim.y * kPqPlainBlock) {
    uint64_t v;
    if (in_width == 0) {
      v = (p[j >> 3] >> (j & 7)) & 1;
    } else if (big_endian) {
      const uint8_t* q = p + j * in_width;
      v = (uint64_t)(int64_t)(int8_t)q[0];
      for (int k = 1; k < in_width; ++k) v = (v << 8) | q[k];
    } else if (in_width == 8) {
      __builtin_memcpy(&v, p + j * 8, 8);
    } else {
      int32_t w;
      __builtin_memcpy(&w, p + j * 4, 4);
      v = (uint64_t)(int64_t)w;
    }
    const int64_t row = map ? map[pg.first_row + j] : pg.first_row + j;
    store_low(out, row, out_width, v);
  }
}

__global__ void __launch_bounds__(WAVE)
pq_rle_values_kernel(const uint8_t* buf, int64_t buf_n, const int64_t* desc,
                     int64_t nrows, const int32_t* map, const int32_t* stored,
                     const uint8_t* dict, int64_t dict_n, uint8_t* out,
                     int out_width, int32_t* status) {
  __shared__ RleRuns runs;
  const int lane = threadIdx.x;
  const PqPage pg =
      load_page(buf, buf_n, desc + (int64_t)blockIdx.x * kPqDesc, nrows);
  if (pg.enc == kEncPlain) return;
  if (pg.err) {
    if (lane == 0) atomicOr(&status[blockIdx.x], pg.err);
    return;
  }
  int64_t n = stored ? stored[blockIdx.x] : pg.nv;
  if (n > pg.nv) n = pg.nv;
  if (n == 0) return;
  int64_t beg = pg.val_beg, end = pg.val_end;
  int bw = 1;
  bool ok = true;
  if (pg.enc == kEncDict) {
    ok = end - beg >= 1;
    if (ok) bw = buf[beg++];
    ok = ok && bw <= 32;
  } else {
    ok = end - beg >= 4;
    if (ok) {
      const int64_t len = le32(buf + beg);
      beg += 4;
      ok = len <= end - beg;
      end = beg + len;
    }
  }
  bool in_range = true;
  if (ok) {
    ok = rle_hybrid(
        buf + beg, end - beg, bw, n, runs, lane,
        [&](int64_t i, uint32_t v, bool active) {
          if (!active) return;
          if ((int64_t)v >= dict_n) {
            in_range = false;
            v = 0;
          }
          const int64_t row = map ? map[pg.first_row + i] : pg.first_row + i;
          if (!dict) {
            store_low(out, row, out_width, v);
          } else if (out_width == 8) {
            ((uint64_t*)out)[row] = ((const uint64_t*)dict)[v];
          } else if (out_width == 4) {
            ((uint32_t*)out)[row] = ((const uint32_t*)dict)[v];
          } else if (out_width == 2) {
            ((uint16_t*)out)[row] = ((const uint16_t*)dict)[v];
          } else {
            out[row] = dict[v];
          }
        });
  }
  if (__ballot(!in_range) != 0) ok = false;
  if (!ok && lane == 0) atomicOr(&status[blockIdx.x], kPqCorrupt);
}

// ---------------------------------------------------------------------------
// the dictionary page of a string column
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE)
pq_dict_strings_kernel(const uint8_t* buf, int64_t buf_n, const int64_t* desc,
                       int64_t n, int64_t* offsets, uint8_t* bytes,
                       int64_t total, int32_t* status) {
  __shared__ __attribute__((aligned(16))) uint8_t win[kPqStage];
  __shared__ uint32_t e_src[WAVE], e_dst[WAVE], e_len[WAVE];
  __shared__ uint32_t ctl[4];  // entries, position, bytes written, error
  const int lane = threadIdx.x;
  const PqPage pg = load_page(buf, buf_n, desc, n);
  if (pg.err || pg.nv != n) {
    if (lane == 0) {
      atomicOr(status, pg.err ? pg.err : kPqBadDesc);
      for (int64_t i = 0; i <= n; ++i) offsets[i] = 0;
    }
    return;
  }
  const uint8_t* p = buf + pg.val_beg;
  const uint32_t len = (uint32_t)(pg.val_end - pg.val_beg);
  uint32_t pos = 0, o = 0;
  int64_t done = 0;
  bool err = false;
  while (done < n && !err) {
    const int64_t abs = pg.val_beg + pos;
    stage_window(buf, buf_n, abs, win, lane);
    __syncthreads();
    if (lane == 0) {
      const uint32_t w0 = (uint32_t)(abs & 15);
      uint32_t c = 0, q = pos, w = o, e = 0;
      while (c < WAVE && done + c < n) {
        const uint32_t wi = w0 + (q - pos);
        if (wi + 4 > kPqStage) break;  // never the window's first entry
        if (len - q < 4) { e = 1; break; }
        const uint32_t l = win[wi] | ((uint32_t)win[wi + 1] << 8) |
                           ((uint32_t)win[wi + 2] << 16) |
                           ((uint32_t)win[wi + 3] << 24);
        if (l > len - q - 4 || (int64_t)w + l > total) { e = 1; break; }
        e_src[c] = q + 4;
        e_dst[c] = w;
        e_len[c] = l;
        offsets[done + c] = w;
        q += 4 + l;
        w += l;
        ++c;
      }
      ctl[0] = c;
      ctl[1] = q;
      ctl[2] = w;
      ctl[3] = e;
    }
    __syncthreads();
    const uint32_t cnt = ctl[0];
    uint32_t l = 0, s = 0, dst = 0;
    if ((uint32_t)lane < cnt) {
      l = e_len[lane];
      s = e_src[lane];
      dst = e_dst[lane];
    }
    if (l < WAVE)
      for (uint32_t i = 0; i < l; ++i) bytes[dst + i] = p[s + i];
    uint64_t longs = __ballot(l >= WAVE);
    while (longs) {
      const int src_lane = __ffsll((unsigned long long)longs) - 1;
      longs &= longs - 1;
      const uint32_t ll = __shfl(l, src_lane, WAVE);
      const uint32_t ss = __shfl(s, src_lane, WAVE);
      const uint32_t dd = __shfl(dst, src_lane, WAVE);
      for (uint32_t i = lane; i < ll; i += WAVE) bytes[dd + i] = p[ss + i];
    }
    done += cnt;
    pos = ctl[1];
    o = ctl[2];
    err = ctl[3] != 0;
    __syncthreads();
  }
  if (!err && (int64_t)o != total) err = true;
  if (lane == 0) {
    if (err) {
      atomicOr(status, kPqCorrupt);
      for (int64_t i = 0; i <= n; ++i) offsets[i] = 0;
    } else {
      offsets[n] = o;
    }
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
namespace {

struct PqArgs {
  int64_t buf_n;
  int64_t pages;
  torch::Device dev;
};

PqArgs check_pages(const char* who, const Tensor& buf, const Tensor& desc,
                   const Tensor& status) {
  TORCH_CHECK(buf.is_cuda(), who, ": buf must be on a GPU device");
  const auto dev = buf.device();
  check_tensor(who, "buf", buf, torch::kUInt8, dev);
  check_tensor(who, "desc", desc, torch::kInt64, dev);
  check_tensor(who, "status", status, torch::kInt32, dev);
  TORCH_CHECK(desc.dim() == 2 && desc.size(1) == kPqDesc, who,
              ": desc must be [pages, ", kPqDesc, "]");
  TORCH_CHECK(status.dim() == 1 && status.numel() == desc.size(0), who,
              ": status must have one entry per page");
  TORCH_CHECK(desc.size(0) <= 65535 * 1024, who, ": too many pages");
  TORCH_CHECK(buf.numel() == 0 ||
                  reinterpret_cast<uintptr_t>(buf.data_ptr()) % 16 == 0,
              who, ": buf must be 16-byte aligned");
  return {buf.numel(), desc.size(0), dev};
}

// optional int32 tensor of `n` entries; null when absent
const int32_t* opt_i32(const char* who, const char* name, const OptTensor& t,
                       int64_t n, const torch::Device& dev) {
  if (!t.has_value()) return nullptr;
  check_tensor(who, name, *t, torch::kInt32, dev);
  TORCH_CHECK(t->numel() == n, who, ": ", name, " must have ", n, " entries");
  return t->data_ptr<int32_t>();
}

int64_t check_out(const char* who, const Tensor& out, int64_t width,
                  const torch::Device& dev) {
  check_tensor(who, "out", out, torch::kUInt8, dev);
  TORCH_CHECK(width == 1 || width == 2 || width == 4 || width == 8, who,
              ": out_width must be 1, 2, 4 or 8");
  TORCH_CHECK(out.numel() % width == 0 &&
                  (out.numel() == 0 ||
                   reinterpret_cast<uintptr_t>(out.data_ptr()) % 8 == 0),
              who, ": out must hold whole, aligned values");
  return out.numel() / width;
}

}  // namespace

void pq_snappy(Tensor buf, Tensor desc, Tensor status) {
  const PqArgs a = check_pages("pq_snappy", buf, desc, status);
  if (a.pages == 0) return;
  hipLaunchKernelGGL(pq_snappy_kernel, dim3((unsigned)a.pages), dim3(WAVE), 0,
                     cur_stream(), buf.data_ptr<uint8_t>(), a.buf_n,
                     desc.data_ptr<int64_t>(), status.data_ptr<int32_t>());
}

std::vector<Tensor> pq_levels(Tensor buf, Tensor desc, int64_t nrows,
                              Tensor status) {
  const PqArgs a = check_pages("pq_levels", buf, desc, status);
  TORCH_CHECK(nrows >= 0 && nrows < INT32_MAX,
              "pq_levels: need 0 <= nrows < 2^31");
  auto validity =
      torch::zeros({nrows}, torch::dtype(torch::kBool).device(a.dev));
  auto map = torch::empty({nrows}, torch::dtype(torch::kInt32).device(a.dev));
  auto stored =
      torch::empty({a.pages}, torch::dtype(torch::kInt32).device(a.dev));
  if (a.pages)
    hipLaunchKernelGGL(pq_levels_kernel, dim3((unsigned)a.pages), dim3(WAVE),
                       0, cur_stream(), bytes_ptr(buf), a.buf_n,
                       desc.data_ptr<int64_t>(), nrows,
                       validity.data_ptr<bool>(), map.data_ptr<int32_t>(),
                       stored.data_ptr<int32_t>(), status.data_ptr<int32_t>());
  return {validity, map, stored};
}

void pq_plain(Tensor buf, Tensor desc, OptTensor map, OptTensor stored,
              Tensor out, int64_t in_width, bool big_endian,
              int64_t out_width, Tensor status) {
  const PqArgs a = check_pages("pq_plain", buf, desc, status);
  const int64_t nrows = check_out("pq_plain", out, out_width, a.dev);
  TORCH_CHECK(big_endian ? (in_width >= 1 && in_width <= 8)
                         : (in_width == 0 || in_width == 4 || in_width == 8),
              "pq_plain: in_width must be 0 (bits), 4 or 8, or 1..8 "
              "big-endian bytes, got ", in_width);
  const int32_t* mp = opt_i32("pq_plain", "map", map, nrows, a.dev);
  const int32_t* st = opt_i32("pq_plain", "stored", stored, a.pages, a.dev);
  TORCH_CHECK((mp == nullptr) == (st == nullptr),
              "pq_plain: map and stored go together");
  if (a.pages == 0 || nrows == 0) return;
  // enough slices for the largest page a row group of `nrows` can hold
  const int64_t per_page = (nrows + a.pages - 1) / a.pages;
  int gy = (int)std::min<int64_t>(
      64, std::max<int64_t>(1, 4 * per_page / (kPqPlainBlock * 8)));
  TORCH_CHECK(a.pages <= INT32_MAX, "pq_plain: too many pages");
  hipLaunchKernelGGL(pq_plain_kernel, dim3((unsigned)a.pages, gy),
                     dim3(kPqPlainBlock), 0, cur_stream(), bytes_ptr(buf),
                     a.buf_n, desc.data_ptr<int64_t>(), nrows, mp, st,
                     out.data_ptr<uint8_t>(), (int)in_width, big_endian,
                     (int)out_width, status.data_ptr<int32_t>());
}

void pq_rle_values(Tensor buf, Tensor desc, OptTensor map, OptTensor stored,
                   OptTensor dict, int64_t dict_n, Tensor out,
                   int64_t out_width, Tensor status) {
  const PqArgs a = check_pages("pq_rle_values", buf, desc, status);
  const int64_t nrows = check_out("pq_rle_values", out, out_width, a.dev);
  const int32_t* mp = opt_i32("pq_rle_values", "map", map, nrows, a.dev);
  const int32_t* st =
      opt_i32("pq_rle_values", "stored", stored, a.pages, a.dev);
  TORCH_CHECK((mp == nullptr) == (st == nullptr),
              "pq_rle_values: map and stored go together");
  TORCH_CHECK(dict_n >= 0, "pq_rle_values: dict_n must not be negative");
  const uint8_t* dp = nullptr;
  if (dict.has_value()) {
    check_tensor("pq_rle_values", "dict", *dict, torch::kUInt8, a.dev);
    TORCH_CHECK(dict->numel() == dict_n * out_width &&
                    (dict_n == 0 ||
                     reinterpret_cast<uintptr_t>(dict->data_ptr()) % 8 == 0),
                "pq_rle_values: dict must hold dict_n aligned values of "
                "out_width bytes");
    dp = bytes_ptr(*dict);
  }
  if (a.pages == 0 || nrows == 0) return;
  hipLaunchKernelGGL(pq_rle_values_kernel, dim3((unsigned)a.pages), dim3(WAVE),
                     0, cur_stream(), bytes_ptr(buf), a.buf_n,
                     desc.data_ptr<int64_t>(), nrows, mp, st, dp, dict_n,
                     out.data_ptr<uint8_t>(), (int)out_width,
                     status.data_ptr<int32_t>());
}

std::vector<Tensor> pq_dict_strings(Tensor buf, Tensor desc, int64_t n,
                                    int64_t total, Tensor status) {
  const PqArgs a = check_pages("pq_dict_strings", buf, desc, status);
  TORCH_CHECK(a.pages == 1, "pq_dict_strings: desc must be the one row of "
                            "the dictionary page");
  TORCH_CHECK(n >= 0 && n < kPqMaxPage && total >= 0 && total < kPqMaxPage,
              "pq_dict_strings: n and total must be in [0, 2^30)");
  auto offsets =
      torch::empty({n + 1}, torch::dtype(torch::kInt64).device(a.dev));
  auto bytes = torch::empty({total}, torch::dtype(torch::kUInt8).device(a.dev));
  hipLaunchKernelGGL(pq_dict_strings_kernel, dim3(1), dim3(WAVE), 0,
                     cur_stream(), bytes_ptr(buf), a.buf_n,
                     desc.data_ptr<int64_t>(), n, offsets.data_ptr<int64_t>(),
                     total ? bytes.data_ptr<uint8_t>() : nullptr, total,
                     status.data_ptr<int32_t>());
  return {offsets, bytes};
}
