// Byte helpers shared by the text scanners (csv.hip, json.hip): a thread's 16
// bytes of a 4096-byte tile as two words, masks over them, and the UTF-8
// evidence both scanners collect per tile.
#pragma once

#include "common.h"

// ---------------------------------------------------------------------------
// 16 bytes of a thread
// ---------------------------------------------------------------------------
struct Bytes16 {
  uint64_t lo, hi;
};

// data[base, base + 16) with zeros from n on; base is a multiple of 16 and
// data is 16-byte aligned
DEV_INLINE Bytes16 load16(const uint8_t* data, int64_t n, int64_t base) {
  Bytes16 b{0, 0};
  if (base + 16 <= n) {
    uint4 v = *(const uint4*)(data + base);
    b.lo = v.x | ((uint64_t)v.y << 32);
    b.hi = v.z | ((uint64_t)v.w << 32);
  } else {
    for (int i = 0; i < 8 && base + i < n; ++i)
      b.lo |= (uint64_t)data[base + i] << (8 * i);
    for (int i = 8; i < 16 && base + i < n; ++i)
      b.hi |= (uint64_t)data[base + i] << (8 * (i - 8));
  }
  return b;
}

DEV_INLINE uint32_t byte_of(const Bytes16& b, int i) {
  return (uint32_t)((i < 8 ? b.lo >> (8 * i) : b.hi >> (8 * (i - 8))) & 0xFF);
}

DEV_INLINE uint32_t eq_mask(const Bytes16& b, uint32_t c) {
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) m |= (uint32_t)(byte_of(b, i) == c) << i;
  return m;
}

DEV_INLINE int wave_sum(int v) {
  for (int off = WAVE / 2; off; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// UTF-8 evidence of the thread's 16 bytes at `base` (b is zero from n on):
// every lead byte checks its own continuation bytes and the overlong,
// surrogate and > U+10FFFF ranges of the first one, looking up to 3 bytes past
// the 16 (bounded global reads).  *diff gets continuation bytes claimed by
// leads minus those present; the return value is true for a byte that cannot
// stand where it is.  A character cut off by the chunk's end is tolerated.
DEV_INLINE bool utf8_evidence(const uint8_t* data, int64_t n, int64_t base,
                              const Bytes16& b, int* diff_out) {
  uint32_t nx = 0;  // the 3 bytes after the thread's 16
  if (base < n) {
    if ((b.hi >> 40) & 0x808080) {  // the last three bytes are not all ASCII
      for (int j = 0; j < 3; ++j)
        if (base + 16 + j < n) nx |= (uint32_t)data[base + 16 + j] << (8 * j);
    }
  }
  int diff = 0;
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    uint32_t c = byte_of(b, i);
    if (c < 0x80) continue;
    if (c < 0xC0) {
      --diff;
      continue;
    }
    int k = c < 0xE0 ? 1 : c < 0xF0 ? 2 : 3;
    uint32_t lo = c == 0xE0 ? 0xA0 : c == 0xF0 ? 0x90 : 0x80;
    uint32_t hi = c == 0xED ? 0x9F : c == 0xF4 ? 0x8F : 0xBF;
    if (c < 0xC2 || c > 0xF4) bad = true;
#pragma unroll
    for (int j = 1; j <= 3; ++j) {
      if (j > k || base + i + j >= n) continue;  // cut off by the chunk end
      int at = i + j;
      uint32_t cb = at < 16 ? byte_of(b, at < 16 ? at : 0)
                            : (nx >> (8 * (at - 16))) & 0xFF;
      ++diff;
      if (cb < (j == 1 ? lo : 0x80u) || cb > (j == 1 ? hi : 0xBFu)) bad = true;
    }
  }
  *diff_out = diff;
  return bad;
}
