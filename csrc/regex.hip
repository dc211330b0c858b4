// Boolean regex / LIKE matching by table-driven DFA (gfx950).  The tables
// come from daft_amd/kernels/regex_dfa.py, whose Program.match_host walks
// them the same way: one lookup per input byte, no backtracking.
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
