// String kernels over Arrow offsets+bytes (gfx950) — the GPU equivalents of
// the reference's daft-functions-utf8 kernels.  One thread per row for
// predicate/search ops (TPC-H string rows are short); byte-parallel for
// case mapping.
#include "common.h"
#include "host_args.h"
#include "api.h"

// mode: 0 = find (first match position, -1 if none)
//       1 = prefix test (0 or -1)
//       2 = suffix test (0 or -1)
__global__ void str_find_kernel(const int64_t* offs, const uint8_t* bytes,
                                int64_t n, const uint8_t* pat, int64_t plen,
                                int mode, int64_t* out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t a = offs[i], b = offs[i + 1];
    int64_t len = b - a;
    const uint8_t* s = bytes + a;
    int64_t res = -1;
    if (plen == 0) {
      res = 0;
    } else if (len >= plen) {
      if (mode == 1) {
        bool ok = true;
        for (int64_t j = 0; j < plen; ++j)
          if (s[j] != pat[j]) { ok = false; break; }
        res = ok ? 0 : -1;
      } else if (mode == 2) {
        bool ok = true;
        const uint8_t* t = s + len - plen;
        for (int64_t j = 0; j < plen; ++j)
          if (t[j] != pat[j]) { ok = false; break; }
        res = ok ? 0 : -1;
      } else {
        for (int64_t p = 0; p + plen <= len; ++p) {
          if (s[p] != pat[0]) continue;
          bool ok = true;
          for (int64_t j = 1; j < plen; ++j)
            if (s[p + j] != pat[j]) { ok = false; break; }
          if (ok) { res = p; break; }
        }
      }
    }
    out[i] = res;
  }
}

Tensor str_find(Tensor offsets, Tensor bytes, Tensor pattern, int64_t mode) {
  StrCol c = check_strcol("str_find", offsets, bytes);
  auto dev = offsets.device();
  check_tensor("str_find", "pattern", pattern, torch::kUInt8, dev);
  auto out = torch::empty({c.n}, torch::dtype(torch::kInt64).device(dev));
  if (c.n > 0) {
    int block = 256;
    hipLaunchKernelGGL(str_find_kernel, dim3(grid_1d(c.n, block)),
                       dim3(block), 0, cur_stream(), c.offs, c.bytes, c.n,
                       bytes_ptr(pattern), pattern.numel(), (int)mode,
                       out.data_ptr<int64_t>());
  }
  return out;
}

// ordered multi-substring LIKE (patterns without '_'): needles concatenated
// in `blob` with lengths in `lens`; anchored prefix/suffix flags.
__global__ void str_like_kernel(const int64_t* offs, const uint8_t* bytes,
                                int64_t n, const uint8_t* blob,
                                const int64_t* lens, int nneedles,
                                bool anchored_prefix, bool anchored_suffix,
                                bool* out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t a = offs[i], b = offs[i + 1];
    int64_t len = b - a;
    const uint8_t* s = bytes + a;
    bool ok = true;
    int64_t pos = 0;
    int64_t blob_off = 0;
    for (int k = 0; k < nneedles && ok; ++k) {
      const uint8_t* nd = blob + blob_off;
      int64_t nl = lens[k];
      blob_off += nl;
      bool is_first = (k == 0), is_last = (k == nneedles - 1);
      if (is_first && anchored_prefix) {
        if (len < nl) { ok = false; break; }
        for (int64_t j = 0; j < nl; ++j)
          if (s[j] != nd[j]) { ok = false; break; }
        pos = nl;
        continue;
      }
      if (is_last && anchored_suffix) {
        if (len - pos < nl) { ok = false; break; }
        const uint8_t* t = s + len - nl;
        for (int64_t j = 0; j < nl; ++j)
          if (t[j] != nd[j]) { ok = false; break; }
        continue;
      }
      // search nd in s[pos..]
      int64_t found = -1;
      for (int64_t p = pos; p + nl <= len; ++p) {
        if (s[p] != nd[0]) continue;
        bool m = true;
        for (int64_t j = 1; j < nl; ++j)
          if (s[p + j] != nd[j]) { m = false; break; }
        if (m) { found = p; break; }
      }
      if (found < 0) { ok = false; break; }
      pos = found + nl;
    }
    out[i] = ok;
  }
}

Tensor str_like(Tensor offsets, Tensor bytes, Tensor needles, Tensor lens,
                bool anchored_prefix, bool anchored_suffix) {
  StrCol c = check_strcol("str_like", offsets, bytes);
  auto dev = offsets.device();
  check_tensor("str_like", "needles", needles, torch::kUInt8, dev);
  check_tensor("str_like", "lens", lens, torch::kInt64, dev);
  auto out = torch::empty({c.n}, torch::dtype(torch::kBool).device(dev));
  if (c.n > 0) {
    int block = 256;
    hipLaunchKernelGGL(str_like_kernel, dim3(grid_1d(c.n, block)),
                       dim3(block), 0, cur_stream(), c.offs, c.bytes, c.n,
                       bytes_ptr(needles), lens.data_ptr<int64_t>(),
                       (int)lens.numel(), anchored_prefix, anchored_suffix,
                       out.data_ptr<bool>());
  }
  return out;
}

// ASCII case mapping, byte-parallel (UTF-8 multibyte left untouched).
__global__ void str_case_kernel(const uint8_t* in, int64_t nbytes, int mode,
                                uint8_t* out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nbytes;
       i += stride) {
    uint8_t c = in[i];
    if (mode == 0) {  // lower
      if (c >= 'A' && c <= 'Z') c += 32;
    } else {
      if (c >= 'a' && c <= 'z') c -= 32;
    }
    out[i] = c;
  }
}

Tensor str_case(Tensor offsets, Tensor bytes, int64_t mode) {
  StrCol c = check_strcol("str_case", offsets, bytes);
  auto out = torch::empty_like(bytes);
  if (c.nbytes > 0) {
    int block = 256;
    hipLaunchKernelGGL(str_case_kernel, dim3(grid_1d(c.nbytes, block)),
                       dim3(block), 0, cur_stream(), c.bytes, c.nbytes,
                       (int)mode, out.data_ptr<uint8_t>());
  }
  return out;
}

// The one UTF-8 walk: byte offset in s[0, len) of code point `k`, or `len`
// when the row has fewer; *seen = code points before that offset.  A code
// point starts at every byte that is not a 10xxxxxx continuation byte.
DEV_INLINE int64_t utf8_offset_of_char(const uint8_t* s, int64_t len,
                                       int64_t k, int64_t* seen) {
  int64_t cnt = 0, j = 0;
  for (; j < len; ++j) {
    if ((s[j] & 0xC0) != 0x80) {
      if (cnt == k) break;
      ++cnt;
    }
  }
  *seen = cnt;
  return j;
}

// Per row: where the substring starts in src_bytes and how many bytes it
// has.  start >= 0; length < 0 means to the end of the row.  by_char counts
// code points (STRING), otherwise bytes (BINARY).
__global__ void substr_bounds_kernel(const int64_t* offs,
                                     const uint8_t* bytes, int64_t n,
                                     int64_t start, int64_t length,
                                     bool by_char, int64_t* src_start,
                                     int64_t* out_len) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t a = offs[i], len = offs[i + 1] - a;
    int64_t bs, bl;
    if (by_char) {
      int64_t seen;
      bs = utf8_offset_of_char(bytes + a, len, start, &seen);
      bl = length < 0 ? len - bs
                      : utf8_offset_of_char(bytes + a + bs, len - bs, length,
                                            &seen);
    } else {
      bs = min(start, len);
      bl = length < 0 ? len - bs : min(length, len - bs);
    }
    src_start[i] = a + bs;
    out_len[i] = bl;
  }
}

// Ragged byte copy: out[out_offs[j] + t] = src[seg_start[j] + t].  One thread
// per output byte; it finds its segment by binary search over out_offs (the
// last j with out_offs[j] <= byte), which steps over empty segments.  A
// position outside src reads as 0.
__global__ void copy_segments_kernel(const uint8_t* src, int64_t src_len,
                                     const int64_t* seg_start,
                                     const int64_t* out_offs, int64_t k,
                                     int64_t total, uint8_t* out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    int64_t lo = 0, hi = k;  // out_offs[lo] <= t < out_offs[hi]
    while (hi - lo > 1) {
      int64_t mid = lo + (hi - lo) / 2;
      if (out_offs[mid] <= t) lo = mid; else hi = mid;
    }
    int64_t at = seg_start[lo] + (t - out_offs[lo]);
    out[t] = (at >= 0 && at < src_len) ? src[at] : 0;
  }
}

void launch_copy_segments(const uint8_t* src, int64_t src_len,
                          const int64_t* seg_start, const int64_t* out_offs,
                          int64_t k, int64_t total, uint8_t* out) {
  if (total <= 0) return;
  int block = 256;
  hipLaunchKernelGGL(copy_segments_kernel, dim3(grid_1d(total, block)),
                     dim3(block), 0, cur_stream(), src, src_len, seg_start,
                     out_offs, k, total, out);
}

Tensor copy_segments(Tensor src, Tensor seg_start, Tensor out_offsets) {
  StrCol c = check_strcol("copy_segments", out_offsets, src);
  check_tensor("copy_segments", "seg_start", seg_start, torch::kInt64,
               src.device());
  TORCH_CHECK(seg_start.dim() == 1 && seg_start.numel() == c.n,
              "copy_segments: out_offsets must have one entry more than "
              "seg_start [k]");
  int64_t total = c.n ? out_offsets[c.n].item<int64_t>() : 0;
  TORCH_CHECK(total >= 0 && (c.n == 0 || out_offsets[0].item<int64_t>() == 0),
              "copy_segments: out_offsets must run from 0 to the output size");
  auto out = torch::empty({total},
                          torch::dtype(torch::kUInt8).device(src.device()));
  launch_copy_segments(c.bytes, c.nbytes, seg_start.data_ptr<int64_t>(),
                       c.offs, c.n, total, out.data_ptr<uint8_t>());
  return out;
}

std::vector<Tensor> str_substr(Tensor offsets, Tensor bytes, int64_t start,
                               int64_t length, bool by_char) {
  TORCH_CHECK(start >= 0, "str_substr: start must be >= 0, got ", start);
  StrCol c = check_strcol("str_substr", offsets, bytes);
  auto opts64 = torch::dtype(torch::kInt64).device(offsets.device());
  auto src_start = torch::empty({c.n}, opts64);
  auto new_lens = torch::empty({c.n}, opts64);
  int block = 256;
  if (c.n > 0)
    hipLaunchKernelGGL(substr_bounds_kernel, dim3(grid_1d(c.n, block)),
                       dim3(block), 0, cur_stream(), c.offs, c.bytes, c.n,
                       start, length, by_char, src_start.data_ptr<int64_t>(),
                       new_lens.data_ptr<int64_t>());
  auto [out_off, total] = offsets_from_lens(new_lens);
  auto out = torch::empty({total}, bytes.options());
  launch_copy_segments(c.bytes, c.nbytes, src_start.data_ptr<int64_t>(),
                       out_off.data_ptr<int64_t>(), c.n, total,
                       out.data_ptr<uint8_t>());
  return {out_off, out};
}

// row-wise concat of K string columns
__global__ void str_concat_kernel(const int64_t* const* offs,
                                  const uint8_t* const* datas, int k,
                                  const int64_t* out_off, int64_t n,
                                  uint8_t* out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t pos = out_off[i];
    for (int c = 0; c < k; ++c) {
      int64_t a = offs[c][i], b = offs[c][i + 1];
      const uint8_t* s = datas[c] + a;
      for (int64_t j = 0; j < b - a; ++j) out[pos++] = s[j];
    }
  }
}

std::vector<Tensor> str_concat(const std::vector<Tensor>& offsets,
                               const std::vector<Tensor>& bytes) {
  TORCH_CHECK(!offsets.empty() && offsets.size() == bytes.size(),
              "str_concat: needs at least one column, and as many offsets "
              "as bytes tensors");
  int k = (int)offsets.size();
  StrCol first = check_strcol("str_concat", offsets[0], bytes[0]);
  auto dev = offsets[0].device();
  int64_t n = first.n;
  // column pointers, staged on the host and copied over only if launched
  auto hoffs = torch::empty({k}, torch::dtype(torch::kInt64));
  auto hdata = torch::empty({k}, torch::dtype(torch::kInt64));
  auto lens = torch::zeros({n}, torch::dtype(torch::kInt64).device(dev));
  for (int c = 0; c < k; ++c) {
    StrCol col = check_strcol_rows("str_concat", offsets[c], bytes[c], n, dev);
    hoffs[c] = (int64_t)col.offs;
    hdata[c] = (int64_t)col.bytes;
    lens += offsets[c].slice(0, 1) - offsets[c].slice(0, 0, n);
  }
  auto [out_off, total] = offsets_from_lens(lens);
  auto out = torch::empty({total}, torch::dtype(torch::kUInt8).device(dev));
  if (total > 0) {
    auto doffs = hoffs.to(dev);
    auto ddata = hdata.to(dev);
    int block = 256;
    hipLaunchKernelGGL(str_concat_kernel, dim3(grid_1d(n, block)),
                       dim3(block), 0, cur_stream(),
                       (const int64_t* const*)doffs.data_ptr<int64_t>(),
                       (const uint8_t* const*)ddata.data_ptr<int64_t>(), k,
                       out_off.data_ptr<int64_t>(), n,
                       out.data_ptr<uint8_t>());
  }
  return {out_off, out};
}

__global__ void char_length_kernel(const int64_t* offs, const uint8_t* bytes,
                                   int64_t n, int64_t* out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t a = offs[i], b = offs[i + 1];
    int64_t cnt;
    utf8_offset_of_char(bytes + a, b - a, INT64_MAX, &cnt);
    out[i] = cnt;
  }
}

Tensor str_char_length(Tensor offsets, Tensor bytes) {
  StrCol c = check_strcol("str_char_length", offsets, bytes);
  auto out = torch::zeros(
      {c.n}, torch::dtype(torch::kInt64).device(offsets.device()));
  if (c.n > 0) {
    int block = 256;
    hipLaunchKernelGGL(char_length_kernel, dim3(grid_1d(c.n, block)),
                       dim3(block), 0, cur_stream(), c.offs, c.bytes, c.n,
                       out.data_ptr<int64_t>());
  }
  return out;
}

__global__ void string_compare_kernel(const int64_t* ao, const uint8_t* ab,
                                      const int64_t* bo, const uint8_t* bb,
                                      int64_t n, int8_t* out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t sa = ao[i], ea = ao[i + 1];
    int64_t sb = bo[i], eb = bo[i + 1];
    int64_t la = ea - sa, lb = eb - sb;
    int64_t m = min(la, lb);
    int8_t r = 0;
    for (int64_t j = 0; j < m; ++j) {
      uint8_t x = ab[sa + j], y = bb[sb + j];
      if (x != y) { r = x < y ? -1 : 1; break; }
    }
    if (r == 0 && la != lb) r = la < lb ? -1 : 1;
    out[i] = r;
  }
}

Tensor string_compare(Tensor a_off, Tensor a_bytes, Tensor b_off,
                      Tensor b_bytes) {
  StrCol a = check_strcol("string_compare", a_off, a_bytes);
  auto dev = a_off.device();
  StrCol b = check_strcol_rows("string_compare", b_off, b_bytes, a.n, dev);
  auto out = torch::zeros({a.n}, torch::dtype(torch::kInt8).device(dev));
  if (a.n > 0) {
    int block = 256;
    hipLaunchKernelGGL(string_compare_kernel, dim3(grid_1d(a.n, block)),
                       dim3(block), 0, cur_stream(), a.offs, a.bytes, b.offs,
                       b.bytes, a.n, out.data_ptr<int8_t>());
  }
  return out;
}
