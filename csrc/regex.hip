// Boolean regex / LIKE matching by table-driven DFA (gfx950).  The tables
// come from daft_amd/kernels/regex_dfa.py, whose Program.match_host walks
// them the same way: one lookup per input byte, no backtracking.  Below it,
// match positions (count / spans) from SpanProgram's forward and reverse
// tables (strings.hip's copy_segments assembles extract / replace / split
// results from those spans).
#include "common.h"
#include "host_args.h"
#include "api.h"

// state flags, shared with regex_dfa.py
constexpr uint8_t kRxMatched = 1;  // sticky: True whatever follows
constexpr uint8_t kRxEnd = 2;      // True if the row ends in this state
constexpr uint8_t kRxDead = 4;     // no continuation can match

// the launcher refuses programs whose tables do not fit one block's LDS
constexpr int64_t kRxMaxLdsBytes = 64 * 1024;

// Every thread of the block copies its share of one automaton into LDS:
// table, then byte_class (skipped when null), then flags.  The caller's
// single __syncthreads() follows.
DEV_INLINE void stage_automaton(int16_t* l_table, const int16_t* table,
                                int table_len, uint8_t* l_class,
                                const uint8_t* byte_class, uint8_t* l_flags,
                                const uint8_t* flags, int n_states) {
  for (int j = threadIdx.x; j < table_len; j += blockDim.x)
    l_table[j] = table[j];
  if (byte_class != nullptr)
    for (int j = threadIdx.x; j < 256; j += blockDim.x)
      l_class[j] = byte_class[j];
  for (int j = threadIdx.x; j < n_states; j += blockDim.x)
    l_flags[j] = flags[j];
}

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
  stage_automaton(l_table, table, table_len, l_class, byte_class, l_flags,
                  flags, n_states);
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
  stage_automaton(l_fwd, fwd_table, fwd_len, l_class, byte_class, l_fflags,
                  fwd_flags, fwd_states);
  if (kSpans)
    stage_automaton(l_rev, rev_table, rev_len, nullptr, nullptr, l_rflags,
                    rev_flags, rev_states);
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
  StrCol col;
  const bool* valid;
  int64_t fwd_states, rev_states, lds_bytes;
};

// Everything a DFA launch depends on, checked on the host before any
// launch.  `rev_table` / `rev_flags` are null for regex_match and
// regex_count.
SpanArgs check_span_program(const char* who, const Tensor& offsets,
                            const Tensor& bytes, const OptTensor& valid,
                            const Tensor& fwd_table, const Tensor& byte_class,
                            const Tensor& fwd_flags, int64_t n_classes,
                            int64_t start, const Tensor* rev_table,
                            const Tensor* rev_flags, int64_t rev_start,
                            int64_t limit) {
  SpanArgs r;
  r.col = check_strcol(who, offsets, bytes);
  auto dev = offsets.device();
  r.valid = check_valid(who, valid, r.col.n, dev);
  check_tensor(who, "fwd_table", fwd_table, torch::kInt16, dev);
  check_tensor(who, "byte_class", byte_class, torch::kUInt8, dev);
  TORCH_CHECK(byte_class.numel() == 256, who,
              ": byte_class must have 256 entries");
  check_tensor(who, "fwd_flags", fwd_flags, torch::kUInt8, dev);
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
    check_tensor(who, "rev_table", *rev_table, torch::kInt16, dev);
    check_tensor(who, "rev_flags", *rev_flags, torch::kUInt8, dev);
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

Tensor regex_match(Tensor offsets, Tensor bytes, Tensor table,
                   Tensor byte_class, Tensor flags, int64_t n_classes,
                   int64_t start) {
  SpanArgs r = check_span_program("regex_match", offsets, bytes, c10::nullopt,
                                  table, byte_class, flags, n_classes, start,
                                  nullptr, nullptr, 0, -1);
  int64_t n = r.col.n;
  auto out = torch::empty(
      {n}, torch::dtype(torch::kBool).device(offsets.device()));
  if (n > 0) {
    int block = 256;
    hipLaunchKernelGGL(regex_match_kernel, dim3(grid_1d(n, block)),
                       dim3(block), (size_t)r.lds_bytes, cur_stream(),
                       r.col.offs, r.col.bytes, n, table.data_ptr<int16_t>(),
                       byte_class.data_ptr<uint8_t>(),
                       flags.data_ptr<uint8_t>(), (int)table.numel(),
                       (int)r.fwd_states, (int)n_classes, (int)start,
                       out.data_ptr<bool>());
  }
  return out;
}

Tensor regex_count(Tensor offsets, Tensor bytes, OptTensor valid,
                   Tensor fwd_table, Tensor byte_class, Tensor fwd_flags,
                   int64_t n_classes, int64_t start, int64_t limit) {
  SpanArgs r = check_span_program("regex_count", offsets, bytes, valid,
                                  fwd_table, byte_class, fwd_flags, n_classes,
                                  start, nullptr, nullptr, 0, limit);
  int64_t n = r.col.n;
  auto out = torch::empty(
      {n}, torch::dtype(torch::kInt64).device(offsets.device()));
  if (n > 0) {
    int block = 256;
    hipLaunchKernelGGL(
        regex_span_kernel<false>, dim3(grid_1d(n, block)), dim3(block),
        (size_t)r.lds_bytes, cur_stream(), r.col.offs, r.col.bytes,
        r.col.nbytes, r.valid, n, fwd_table.data_ptr<int16_t>(),
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
  int64_t n = r.col.n;
  auto dev = offsets.device();
  check_tensor("regex_spans", "match_offsets", match_offsets, torch::kInt64,
               dev);
  TORCH_CHECK(match_offsets.numel() == n + 1,
              "regex_spans: match_offsets must have n + 1 entries");
  int64_t m = match_offsets[n].item<int64_t>();
  TORCH_CHECK(m >= 0, "regex_spans: match_offsets must end at the number of "
                      "matches, got ", m);
  auto opts = torch::dtype(torch::kInt64).device(dev);
  // a slot the kernel leaves alone (match_offsets promised more matches
  // than the row has) reads as the empty span at 0
  auto starts = torch::zeros({m}, opts);
  auto ends = torch::zeros({m}, opts);
  if (n > 0 && m > 0) {
    int block = 256;
    hipLaunchKernelGGL(
        regex_span_kernel<true>, dim3(grid_1d(n, block)), dim3(block),
        (size_t)r.lds_bytes, cur_stream(), r.col.offs, r.col.bytes,
        r.col.nbytes, r.valid, n, fwd_table.data_ptr<int16_t>(),
        rev_table.data_ptr<int16_t>(), byte_class.data_ptr<uint8_t>(),
        fwd_flags.data_ptr<uint8_t>(), rev_flags.data_ptr<uint8_t>(),
        (int)fwd_table.numel(), (int)rev_table.numel(), (int)r.fwd_states,
        (int)r.rev_states, (int)n_classes, (int)start, (int)rev_start, limit,
        match_offsets.data_ptr<int64_t>(), m, (int64_t*)nullptr,
        starts.data_ptr<int64_t>(), ends.data_ptr<int64_t>());
  }
  return {starts, ends};
}
