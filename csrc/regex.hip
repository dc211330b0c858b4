// Boolean regex / LIKE matching by table-driven DFA (gfx950).  The tables
// come from daft_amd/kernels/regex_dfa.py, whose Program.match_host walks
// them the same way: one lookup per input byte, no backtracking.  Below it,
// match positions (count / spans) from SpanProgram's forward and reverse
// tables, and the ragged byte copy that assembles extract / replace / split
// results from those spans.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "api.h"

static hipStream_t rx_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// state flags, shared with regex_dfa.py
constexpr uint8_t kRxMatched = 1;  // sticky: True whatever follows
constexpr uint8_t kRxEnd = 2;      // True if the row ends in this state
constexpr uint8_t kRxDead = 4;     // no continuation can match

// the launcher refuses programs whose tables do not fit one block's LDS
constexpr int64_t kRxMaxLdsBytes = 64 * 1024;

// LDS image: table (int16 [n_states * n_classes]) | byte_class (256) | flags.
// One thread per row, as str_find_kernel / str_like_kernel: rows are short.
__global__ void regex_match_kernel(const int64_t* offs, const uint8_t* bytes,
                                   int64_t n, const int16_t* table,
                                   const uint8_t* byte_class,
                                   const uint8_t* flags, int table_len,
                                   int n_states, int n_classes, int start,
                                   bool* out) {
  extern __shared__ int16_t rx_lds[];
  int16_t* l_table = rx_lds;
  uint8_t* l_class = reinterpret_cast<uint8_t*>(rx_lds + table_len);
  uint8_t* l_flags = l_class + 256;
  for (int j = threadIdx.x; j < table_len; j += blockDim.x)
    l_table[j] = table[j];
  for (int j = threadIdx.x; j < 256; j += blockDim.x)
    l_class[j] = byte_class[j];
  for (int j = threadIdx.x; j < n_states; j += blockDim.x)
    l_flags[j] = flags[j];
  __syncthreads();  // reached by every thread, with or without a row

  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t a = offs[i], b = offs[i + 1];
    int s = start;
    uint8_t f = l_flags[s];
    for (int64_t p = a; p < b && !(f & (kRxMatched | kRxDead)); ++p) {
      s = l_table[s * n_classes + l_class[bytes[p]]];
      f = l_flags[s];
    }
    out[i] = (f & kRxMatched) || (f & kRxEnd);
  }
}

// ---------------------------------------------------------------------------
// match spans (regex_dfa.py SpanProgram, whose _walk is this loop in Python)
// ---------------------------------------------------------------------------

constexpr uint8_t kRxSpanMatch = 1;  // fwd: a match ends on entering this
                                     // state; rev: one starts here

// LDS image: fwd table | rev table (int16 each) | byte_class (256) |
// fwd flags | rev flags.  kSpans = false is regexp_count: no reverse
// automaton is staged or walked, and only `counts` is written.
//
// Per row, from p = row start: walk the forward automaton, remembering the
// last position at which it entered a match state, until it is dead or the
// row ends; that position is the end of the leftmost-first match.  Walk the
// reverse automaton back from there to p; the smallest accepting position
// is the start.  Search again from the end.  Matches are never empty, so
// every round advances p.
template <bool kSpans>
__global__ void regex_span_kernel(
    const int64_t* offs, const uint8_t* bytes, int64_t nbytes,
    const bool* valid, int64_t n, const int16_t* fwd_table,
    const int16_t* rev_table, const uint8_t* byte_class,
    const uint8_t* fwd_flags, const uint8_t* rev_flags, int fwd_len,
    int rev_len, int fwd_states, int rev_states, int n_classes, int start,
    int rev_start, int64_t limit, const int64_t* match_offs, int64_t m,
    int64_t* counts, int64_t* starts, int64_t* ends) {
  extern __shared__ int16_t rx_lds[];
  int16_t* l_fwd = rx_lds;
  int16_t* l_rev = l_fwd + fwd_len;
  uint8_t* l_class = reinterpret_cast<uint8_t*>(l_rev + rev_len);
  uint8_t* l_fflags = l_class + 256;
  uint8_t* l_rflags = l_fflags + fwd_states;
  for (int j = threadIdx.x; j < fwd_len; j += blockDim.x)
    l_fwd[j] = fwd_table[j];
  for (int j = threadIdx.x; j < 256; j += blockDim.x)
    l_class[j] = byte_class[j];
  for (int j = threadIdx.x; j < fwd_states; j += blockDim.x)
    l_fflags[j] = fwd_flags[j];
  if (kSpans) {
    for (int j = threadIdx.x; j < rev_len; j += blockDim.x)
      l_rev[j] = rev_table[j];
    for (int j = threadIdx.x; j < rev_states; j += blockDim.x)
      l_rflags[j] = rev_flags[j];
  }
  __syncthreads();  // reached by every thread, with or without a row

  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t a = offs[i], b = offs[i + 1];
    if (a < 0) a = 0;
    if (b > nbytes) b = nbytes;
    if (valid != nullptr && !valid[i]) b = a;  // bytes under a null
    int64_t base = 0, room = 0;
    if (kSpans) {
      // never write outside this row's slots, whatever match_offs holds
      base = match_offs[i];
      room = match_offs[i + 1] - base;
      if (base < 0 || room < 0 || base + room > m) room = 0;
      if (limit >= 0 && room > limit) room = limit;
    }
    int64_t cnt = 0;
    int64_t p = a;
    while (p < b && cnt != limit && (!kSpans || cnt < room)) {
      int s = start;
      int64_t last = -1;
      for (int64_t q = p; q < b; ++q) {
        s = l_fwd[s * n_classes + l_class[bytes[q]]];
        uint8_t f = l_fflags[s];
        if (f & kRxSpanMatch) last = q + 1;
        if (f & kRxDead) break;
      }
      if (last < 0) break;
      if (kSpans) {
        int r = rev_start;
        int64_t first = last;
        for (int64_t q = last - 1; q >= p; --q) {
          r = l_rev[r * n_classes + l_class[bytes[q]]];
          uint8_t f = l_rflags[r];
          if (f & kRxSpanMatch) first = q;
          if (f & kRxDead) break;
        }
        starts[base + cnt] = first;
        ends[base + cnt] = last;
      }
      ++cnt;
      p = last;
    }
    if (!kSpans) counts[i] = cnt;
  }
}

namespace {

struct SpanArgs {
  int64_t n, fwd_states, rev_states, lds_bytes;
};

// Everything a span launch depends on, checked on the host before any
// launch.  `rev_table` / `rev_flags` are null for regex_count.
SpanArgs check_span_program(const char* who, const Tensor& offsets,
                            const Tensor& bytes, const OptTensor& valid,
                            const Tensor& fwd_table, const Tensor& byte_class,
                            const Tensor& fwd_flags, int64_t n_classes,
                            int64_t start, const Tensor* rev_table,
                            const Tensor* rev_flags, int64_t rev_start,
                            int64_t limit) {
  TORCH_CHECK(offsets.scalar_type() == torch::kInt64 &&
                  offsets.is_contiguous() && offsets.dim() == 1 &&
                  offsets.numel() >= 1,
              who, ": offsets must be contiguous int64 [n + 1]");
  TORCH_CHECK(bytes.scalar_type() == torch::kUInt8 && bytes.is_contiguous(),
              who, ": bytes must be contiguous uint8");
  TORCH_CHECK(fwd_table.scalar_type() == torch::kInt16 &&
                  fwd_table.is_contiguous(),
              who, ": fwd_table must be contiguous int16");
  TORCH_CHECK(byte_class.scalar_type() == torch::kUInt8 &&
                  byte_class.is_contiguous() && byte_class.numel() == 256,
              who, ": byte_class must be contiguous uint8 [256]");
  TORCH_CHECK(fwd_flags.scalar_type() == torch::kUInt8 &&
                  fwd_flags.is_contiguous(),
              who, ": fwd_flags must be contiguous uint8 [n_states]");
  auto dev = offsets.device();
  TORCH_CHECK(dev.is_cuda() && bytes.device() == dev &&
                  fwd_table.device() == dev && byte_class.device() == dev &&
                  fwd_flags.device() == dev,
              who, ": all tensors must be on one device");
  SpanArgs r;
  r.n = offsets.numel() - 1;
  if (valid.has_value()) {
    TORCH_CHECK(valid->scalar_type() == torch::kBool &&
                    valid->is_contiguous() && valid->numel() == r.n &&
                    valid->device() == dev,
                who, ": valid must be contiguous bool [n] on the device");
  }
  r.fwd_states = fwd_flags.numel();
  TORCH_CHECK(r.fwd_states >= 1 && n_classes >= 1 && n_classes <= 256,
              who, ": bad program shape");
  TORCH_CHECK(r.fwd_states * n_classes == fwd_table.numel(), who,
              ": fwd_table has ", fwd_table.numel(), " entries, expected ",
              r.fwd_states, " x ", n_classes);
  TORCH_CHECK(start >= 0 && start < r.fwd_states, who,
              ": start state out of range");
  TORCH_CHECK(limit == -1 || limit >= 1, who,
              ": limit must be -1 or at least 1");
  r.rev_states = 0;
  r.lds_bytes = fwd_table.numel() * 2 + 256 + r.fwd_states;
  if (rev_table != nullptr) {
    TORCH_CHECK(rev_table->scalar_type() == torch::kInt16 &&
                    rev_table->is_contiguous() && rev_table->device() == dev,
                who, ": rev_table must be contiguous int16 on the device");
    TORCH_CHECK(rev_flags->scalar_type() == torch::kUInt8 &&
                    rev_flags->is_contiguous() && rev_flags->device() == dev,
                who, ": rev_flags must be contiguous uint8 on the device");
    r.rev_states = rev_flags->numel();
    TORCH_CHECK(r.rev_states >= 1 &&
                    r.rev_states * n_classes == rev_table->numel(),
                who, ": rev_table has ", rev_table->numel(),
                " entries, expected ", r.rev_states, " x ", n_classes);
    TORCH_CHECK(rev_start >= 0 && rev_start < r.rev_states, who,
                ": reverse start state out of range");
    r.lds_bytes += rev_table->numel() * 2 + r.rev_states;
  }
  TORCH_CHECK(r.lds_bytes <= kRxMaxLdsBytes, who, ": program needs ",
              r.lds_bytes, " bytes of LDS, limit ", kRxMaxLdsBytes);
  return r;
}

}  // namespace

Tensor regex_count(Tensor offsets, Tensor bytes, OptTensor valid,
                   Tensor fwd_table, Tensor byte_class, Tensor fwd_flags,
                   int64_t n_classes, int64_t start, int64_t limit) {
  SpanArgs r = check_span_program("regex_count", offsets, bytes, valid,
                                  fwd_table, byte_class, fwd_flags, n_classes,
                                  start, nullptr, nullptr, 0, limit);
  auto out = torch::empty(
      {r.n}, torch::dtype(torch::kInt64).device(offsets.device()));
  if (r.n > 0) {
    int block = 256;
    const uint8_t* bp = bytes.numel() ? bytes.data_ptr<uint8_t>() : nullptr;
    const bool* vp = valid.has_value() ? valid->data_ptr<bool>() : nullptr;
    hipLaunchKernelGGL(
        regex_span_kernel<false>, dim3(grid_1d(r.n, block)), dim3(block),
        (size_t)r.lds_bytes, rx_stream(), offsets.data_ptr<int64_t>(), bp,
        (int64_t)bytes.numel(), vp, r.n, fwd_table.data_ptr<int16_t>(),
        (const int16_t*)nullptr, byte_class.data_ptr<uint8_t>(),
        fwd_flags.data_ptr<uint8_t>(), (const uint8_t*)nullptr,
        (int)fwd_table.numel(), 0, (int)r.fwd_states, 0, (int)n_classes,
        (int)start, 0, limit, (const int64_t*)nullptr, (int64_t)0,
        out.data_ptr<int64_t>(), (int64_t*)nullptr, (int64_t*)nullptr);
  }
  return out;
}

std::vector<Tensor> regex_spans(Tensor offsets, Tensor bytes, OptTensor valid,
                                Tensor fwd_table, Tensor byte_class,
                                Tensor fwd_flags, int64_t n_classes,
                                int64_t start, Tensor rev_table,
                                Tensor rev_flags, int64_t rev_start,
                                Tensor match_offsets, int64_t limit) {
  SpanArgs r = check_span_program("regex_spans", offsets, bytes, valid,
                                  fwd_table, byte_class, fwd_flags, n_classes,
                                  start, &rev_table, &rev_flags, rev_start,
                                  limit);
  auto dev = offsets.device();
  TORCH_CHECK(match_offsets.scalar_type() == torch::kInt64 &&
                  match_offsets.is_contiguous() &&
                  match_offsets.numel() == r.n + 1 &&
                  match_offsets.device() == dev,
              "regex_spans: match_offsets must be contiguous int64 [n + 1] "
              "on the device");
  int64_t m = match_offsets[r.n].item<int64_t>();
  TORCH_CHECK(m >= 0, "regex_spans: match_offsets must end at the number of "
                      "matches, got ", m);
  auto opts = torch::dtype(torch::kInt64).device(dev);
  // a slot the kernel leaves alone (match_offsets promised more matches
  // than the row has) reads as the empty span at 0
  auto starts = torch::zeros({m}, opts);
  auto ends = torch::zeros({m}, opts);
  if (r.n > 0 && m > 0) {
    int block = 256;
    const uint8_t* bp = bytes.numel() ? bytes.data_ptr<uint8_t>() : nullptr;
    const bool* vp = valid.has_value() ? valid->data_ptr<bool>() : nullptr;
    hipLaunchKernelGGL(
        regex_span_kernel<true>, dim3(grid_1d(r.n, block)), dim3(block),
        (size_t)r.lds_bytes, rx_stream(), offsets.data_ptr<int64_t>(), bp,
        (int64_t)bytes.numel(), vp, r.n, fwd_table.data_ptr<int16_t>(),
        rev_table.data_ptr<int16_t>(), byte_class.data_ptr<uint8_t>(),
        fwd_flags.data_ptr<uint8_t>(), rev_flags.data_ptr<uint8_t>(),
        (int)fwd_table.numel(), (int)rev_table.numel(), (int)r.fwd_states,
        (int)r.rev_states, (int)n_classes, (int)start, (int)rev_start, limit,
        match_offsets.data_ptr<int64_t>(), m, (int64_t*)nullptr,
        starts.data_ptr<int64_t>(), ends.data_ptr<int64_t>());
  }
  return {starts, ends};
}

// Ragged byte copy: out[out_offs[j] + t] = src[seg_start[j] + t].  One thread
// per output byte; it finds its segment by binary search over out_offs (the
// last j with out_offs[j] <= byte), which steps over empty segments.
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

Tensor copy_segments(Tensor src, Tensor seg_start, Tensor out_offsets) {
  TORCH_CHECK(src.scalar_type() == torch::kUInt8 && src.is_contiguous(),
              "copy_segments: src must be contiguous uint8");
  TORCH_CHECK(seg_start.scalar_type() == torch::kInt64 &&
                  seg_start.is_contiguous() && seg_start.dim() == 1,
              "copy_segments: seg_start must be contiguous int64 [k]");
  TORCH_CHECK(out_offsets.scalar_type() == torch::kInt64 &&
                  out_offsets.is_contiguous() && out_offsets.dim() == 1 &&
                  out_offsets.numel() == seg_start.numel() + 1,
              "copy_segments: out_offsets must be contiguous int64 [k + 1]");
  auto dev = src.device();
  TORCH_CHECK(dev.is_cuda() && seg_start.device() == dev &&
                  out_offsets.device() == dev,
              "copy_segments: all tensors must be on one device");
  int64_t k = seg_start.numel();
  int64_t total = k ? out_offsets[k].item<int64_t>() : 0;
  TORCH_CHECK(total >= 0 && (k == 0 || out_offsets[0].item<int64_t>() == 0),
              "copy_segments: out_offsets must run from 0 to the output size");
  auto out = torch::empty({total}, torch::dtype(torch::kUInt8).device(dev));
  if (total > 0) {
    int block = 256;
    const uint8_t* sp = src.numel() ? src.data_ptr<uint8_t>() : nullptr;
    hipLaunchKernelGGL(copy_segments_kernel, dim3(grid_1d(total, block)),
                       dim3(block), 0, rx_stream(), sp, (int64_t)src.numel(),
                       seg_start.data_ptr<int64_t>(),
                       out_offsets.data_ptr<int64_t>(), k, total,
                       out.data_ptr<uint8_t>());
  }
  return out;
}

Tensor regex_match(Tensor offsets, Tensor bytes, Tensor table,
                   Tensor byte_class, Tensor flags, int64_t n_classes,
                   int64_t start) {
  TORCH_CHECK(offsets.scalar_type() == torch::kInt64 &&
                  offsets.is_contiguous() && offsets.numel() >= 1,
              "regex_match: offsets must be contiguous int64 [n + 1]");
  TORCH_CHECK(bytes.scalar_type() == torch::kUInt8 && bytes.is_contiguous(),
              "regex_match: bytes must be contiguous uint8");
  TORCH_CHECK(table.scalar_type() == torch::kInt16 && table.is_contiguous(),
              "regex_match: table must be contiguous int16");
  TORCH_CHECK(byte_class.scalar_type() == torch::kUInt8 &&
                  byte_class.is_contiguous() && byte_class.numel() == 256,
              "regex_match: byte_class must be contiguous uint8 [256]");
  TORCH_CHECK(flags.scalar_type() == torch::kUInt8 && flags.is_contiguous(),
              "regex_match: flags must be contiguous uint8 [n_states]");
  auto dev = offsets.device();
  TORCH_CHECK(bytes.device() == dev && table.device() == dev &&
                  byte_class.device() == dev && flags.device() == dev,
              "regex_match: all tensors must be on one device");
  int64_t n_states = flags.numel();
  TORCH_CHECK(n_states >= 1 && n_classes >= 1 && n_classes <= 256,
              "regex_match: bad program shape");
  TORCH_CHECK(n_states * n_classes == table.numel(),
              "regex_match: table has ", table.numel(), " entries, expected ",
              n_states, " x ", n_classes);
  TORCH_CHECK(start >= 0 && start < n_states,
              "regex_match: start state out of range");
  int64_t lds_bytes = table.numel() * 2 + 256 + n_states;
  TORCH_CHECK(lds_bytes <= kRxMaxLdsBytes, "regex_match: program needs ",
              lds_bytes, " bytes of LDS, limit ", kRxMaxLdsBytes);

  int64_t n = offsets.numel() - 1;
  auto out = torch::empty({n}, torch::dtype(torch::kBool).device(dev));
  if (n > 0) {
    int block = 256;
    const uint8_t* bp = bytes.numel() ? bytes.data_ptr<uint8_t>() : nullptr;
    hipLaunchKernelGGL(regex_match_kernel, dim3(grid_1d(n, block)),
                       dim3(block), (size_t)lds_bytes, rx_stream(),
                       offsets.data_ptr<int64_t>(), bp, n,
                       table.data_ptr<int16_t>(),
                       byte_class.data_ptr<uint8_t>(),
                       flags.data_ptr<uint8_t>(), (int)table.numel(),
                       (int)n_states, (int)n_classes, (int)start,
                       out.data_ptr<bool>());
  }
  return out;
}
