// Host-side argument handling for the launchers: the current stream, and
// checks that refuse a bad tensor with a RuntimeError before anything is
// launched.  They read host metadata only (dtype, strides, sizes, device),
// never device memory, so they add no sync.  Values that live in device
// memory (offsets that are not monotone or point past `bytes`, indices out
// of range) stay the Python wrappers' responsibility.
#pragma once

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <utility>

inline hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// `t` is a contiguous `dtype` tensor on `dev`
inline void check_tensor(const char* who, const char* name,
                         const torch::Tensor& t, torch::ScalarType dtype,
                         const torch::Device& dev) {
  TORCH_CHECK(t.scalar_type() == dtype && t.is_contiguous() &&
                  t.device() == dev,
              who, ": ", name, " must be contiguous ", dtype, " on ", dev);
}

// data pointer of a uint8 tensor, null when it is empty
inline const uint8_t* bytes_ptr(const torch::Tensor& t) {
  return t.numel() ? t.data_ptr<uint8_t>() : nullptr;
}

// Checked view of an Arrow string column: offsets int64 [n + 1], bytes uint8.
struct StrCol {
  const int64_t* offs;
  const uint8_t* bytes;  // null when the column has no bytes
  int64_t n;
  int64_t nbytes;
};

inline StrCol check_strcol(const char* who, const torch::Tensor& offsets,
                           const torch::Tensor& bytes) {
  TORCH_CHECK(offsets.is_cuda(), who, ": offsets must be on a GPU device");
  TORCH_CHECK(offsets.scalar_type() == torch::kInt64 &&
                  offsets.is_contiguous() && offsets.dim() == 1 &&
                  offsets.numel() >= 1,
              who, ": offsets must be contiguous int64 [n + 1]");
  check_tensor(who, "bytes", bytes, torch::kUInt8, offsets.device());
  return {offsets.data_ptr<int64_t>(), bytes_ptr(bytes), offsets.numel() - 1,
          bytes.numel()};
}

// second and later columns of a launcher: checked, and as long as the first
inline StrCol check_strcol_rows(const char* who, const torch::Tensor& offsets,
                                const torch::Tensor& bytes, int64_t n,
                                const torch::Device& dev) {
  StrCol c = check_strcol(who, offsets, bytes);
  TORCH_CHECK(c.n == n && offsets.device() == dev, who,
              ": every column must have ", n, " rows on ", dev, ", got ", c.n,
              " on ", offsets.device());
  return c;
}

// optional validity: contiguous bool [n] on `dev`; null when absent
inline const bool* check_valid(const char* who,
                               const c10::optional<torch::Tensor>& valid,
                               int64_t n, const torch::Device& dev) {
  if (!valid.has_value()) return nullptr;
  check_tensor(who, "valid", *valid, torch::kBool, dev);
  TORCH_CHECK(valid->numel() == n, who, ": valid must have ", n, " rows");
  return valid->data_ptr<bool>();
}

// {offsets int64 [n + 1] running from 0, their last entry} for row lengths
// `lens` int64 [n].  Reading the total is the one sync.
inline std::pair<torch::Tensor, int64_t> offsets_from_lens(
    const torch::Tensor& lens) {
  int64_t n = lens.numel();
  auto out_off = torch::zeros({n + 1}, lens.options());
  if (n == 0) return {out_off, 0};
  out_off.slice(0, 1).copy_(torch::cumsum(lens, 0));
  return {out_off, out_off[n].item<int64_t>()};
}
