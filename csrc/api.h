// Host-side launcher declarations for the daft_amd HIP kernels.
#pragma once

#include <torch/extension.h>
#include <vector>

using torch::Tensor;
using OptTensor = c10::optional<Tensor>;

// descriptor packing (kernels.hip)
Tensor pack_descs(const std::vector<int64_t>& tags,
                  const std::vector<Tensor>& datas,
                  const std::vector<OptTensor>& offsets,
                  const std::vector<OptTensor>& validities);

// hashing (kernels.hip)
Tensor hash_rows(const std::vector<int64_t>& tags,
                 const std::vector<Tensor>& datas,
                 const std::vector<OptTensor>& offsets,
                 const std::vector<OptTensor>& validities, int64_t n,
                 int64_t seed);

// selection (kernels.hip)
Tensor compact_indices(Tensor mask);
std::vector<Tensor> take_string(Tensor offsets, Tensor bytes, Tensor idx);
Tensor merge_strings(Tensor mask, Tensor t_off, Tensor t_bytes, Tensor f_off,
                     Tensor f_bytes, Tensor out_off);

// groupby (kernels.hip)
std::vector<Tensor> groupby(Tensor hashes, const std::vector<int64_t>& tags,
                            const std::vector<Tensor>& datas,
                            const std::vector<OptTensor>& offsets,
                            const std::vector<OptTensor>& validities);
Tensor dense_first_index(Tensor packed, int64_t rng, int64_t sentinel);
Tensor count_distinct_pairs(Tensor hashes, const std::vector<int64_t>& tags,
                            const std::vector<Tensor>& datas,
                            const std::vector<OptTensor>& offsets,
                            const std::vector<OptTensor>& validities,
                            Tensor gids, int64_t num_groups);

// grouped aggregation (groupagg.hip).  Op codes shared with
// daft_amd/kernels/__init__.py (AGG_*).
enum AggOp : int { AGG_SUM = 0, AGG_MIN = 1, AGG_MAX = 2, AGG_COUNT = 3 };
struct MAggCol {  // one aggregate of grouped_multi_agg, packed as 3 x i64
  const double* data;
  const bool* valid;
  int64_t op;
};
std::vector<Tensor> grouped_agg(Tensor group_ids, int64_t num_groups,
                                Tensor values, Tensor valid, int64_t op);
Tensor grouped_count(Tensor group_ids, int64_t num_groups, Tensor valid);
std::vector<Tensor> grouped_multi_agg(Tensor gids, int64_t num_groups,
                                      std::vector<Tensor> datas,
                                      std::vector<OptTensor> valids,
                                      std::vector<int64_t> ops);

// join (join.hip).  mode: 0 inner, 1 left, 2 semi, 3 anti.
// direct-address: int32 table of rng slots, table[key - mn] = build row or
// -1; returns {table, dup} where dup[0] != 0 reports duplicate build keys
// (only looked for when check_dup).
std::vector<Tensor> dense_join_build(Tensor keys, int64_t mn, int64_t rng,
                                     bool check_dup);
std::vector<Tensor> dense_join_probe(Tensor keys, OptTensor valid, int64_t mn,
                                     Tensor table, int64_t mode);
std::vector<Tensor> join_build(Tensor hashes);
std::vector<Tensor> join_probe(
    Tensor table, Tensor next, Tensor probe_hashes, Tensor build_hashes,
    const std::vector<int64_t>& tags_l, const std::vector<Tensor>& data_l,
    const std::vector<OptTensor>& off_l, const std::vector<OptTensor>& val_l,
    const std::vector<int64_t>& tags_r, const std::vector<Tensor>& data_r,
    const std::vector<OptTensor>& off_r, const std::vector<OptTensor>& val_r,
    int64_t mode, bool need_matched);

// sort (sort.hip)
Tensor radix_argsort(Tensor keys);
Tensor string_chunk_key(Tensor offsets, Tensor bytes, int64_t chunk);

// partition (kernels.hip)
Tensor u64_mod(Tensor hashes, int64_t n_partitions);

// stable one-pass partitioner (partition.hip).  Partition id of row i is
// hashes[i] % P in unsigned 64-bit arithmetic, or splitmix64(hashes[i]) % P
// when remix; 1 <= P <= 256.  Returns {perm int64[n], counts int64[P]}:
// perm lists the rows of partition 0 in ascending order, then partition 1..
std::vector<Tensor> hash_partition(Tensor hashes, int64_t num_partitions,
                                   bool remix);

// as-of probe (asof.hip).  Keys are order-preserving u64 bit patterns held in
// int64 (rowops._order_key_u64).  The right side is already filtered to usable
// rows and stably sorted by (group, key).  Group g owns sorted positions
// [seg_offsets[g], seg_offsets[g+1]).  right_rows[p] is the original right row
// at sorted position p.
// left_gids[i] < 0 means "row i matches nothing".
// Returns int64 [nl]: matched original right row, or -1.
// Checked on the host: dtype, contiguity, device, rank, matching lengths,
// strategy, and that nearest comes with allow_exact.  What lives in device
// memory stays the Python wrapper's job: gids below seg_offsets.numel() - 1,
// and monotone offsets from 0 to right_keys.numel().
Tensor asof_probe(Tensor left_keys, Tensor left_gids, Tensor right_keys,
                  Tensor right_rows, Tensor seg_offsets,
                  int64_t strategy /*0 backward, 1 forward, 2 nearest*/,
                  bool allow_exact, bool float_keys);

// multimodal (multimodal.hip)
Tensor simhash(Tensor offsets, Tensor bytes, int64_t ngram_size);
Tensor minhash(Tensor offsets, Tensor bytes, int64_t num_hashes,
               int64_t ngram_size, Tensor perm_a, Tensor perm_b);
Tensor hll_update(Tensor hashes, Tensor gids, Tensor valid,
                  int64_t num_groups);
Tensor image_resize(Tensor src_bytes, Tensor src_off, Tensor src_h,
                    Tensor src_w, int64_t channels, int64_t out_h,
                    int64_t out_w);

// fused expression interpreter (fusedexpr.hip)
std::vector<Tensor> fused_eval(Tensor prog, Tensor lits,
                               std::vector<Tensor> cols,
                               std::vector<OptTensor> valids,
                               std::vector<int64_t> codes,
                               std::vector<double> scales,
                               std::vector<int64_t> out_codes,
                               std::vector<double> out_scales,
                               std::vector<int64_t> out_need_valid,
                               int64_t n);

// hipRTC JIT for fused expressions (fusedjit.hip)
bool fused_jit_available();
std::vector<Tensor> fused_eval_jit(const std::string& src,
                                   std::vector<Tensor> cols,
                                   std::vector<OptTensor> valids,
                                   std::vector<int64_t> out_codes,
                                   std::vector<int64_t> out_need_valid,
                                   int64_t n);

// BPE tokenize (bpe.hip)
std::vector<Tensor> bpe_encode(Tensor offsets, Tensor bytes, Tensor byte2id,
                               Tensor table_keys, Tensor table_vals);

// edit distance (editdist.hip)
Tensor levenshtein(Tensor a_off, Tensor a_bytes, Tensor b_off,
                   Tensor b_bytes, int64_t max_len);

// strings (strings.hip)
Tensor str_find(Tensor offsets, Tensor bytes, Tensor pattern, int64_t mode);
Tensor str_like(Tensor offsets, Tensor bytes, Tensor needles, Tensor lens,
                bool anchored_prefix, bool anchored_suffix);
Tensor str_case(Tensor offsets, Tensor bytes, int64_t mode);
std::vector<Tensor> str_substr(Tensor offsets, Tensor bytes, int64_t start,
                               int64_t length, bool by_char);
std::vector<Tensor> str_concat(const std::vector<Tensor>& offsets,
                               const std::vector<Tensor>& bytes);
Tensor str_char_length(Tensor offsets, Tensor bytes);
Tensor string_compare(Tensor a_off, Tensor a_bytes, Tensor b_off,
                      Tensor b_bytes);
// out[out_offsets[j] + t] = src[seg_start[j] + t]: uint8 [out_offsets[k]]
Tensor copy_segments(Tensor src, Tensor seg_start, Tensor out_offsets);
// the same copy for launchers that hold checked device pointers: `k`
// segments, `total` output bytes, nothing launched for total == 0
void launch_copy_segments(const uint8_t* src, int64_t src_len,
                          const int64_t* seg_start, const int64_t* out_offs,
                          int64_t k, int64_t total, uint8_t* out);

// text cleanup (strtransform.hip); each returns {out_offsets, out_bytes}.
// str_strip trims Python's str.isspace set, mode 0 both sides, 1 left,
// 2 right.  str_right keeps the last n >= 0 code points.  str_reverse
// reverses by code point.  str_normalize_ascii also returns non_ascii bool
// [n]: a row with a byte >= 0x80 is flagged and left empty for the caller, a
// row where `valid` is false is empty and not flagged; every other row has
// punctuation dropped, A-Z folded and whitespace runs collapsed as asked.
std::vector<Tensor> str_strip(Tensor offsets, Tensor bytes, int64_t mode);
std::vector<Tensor> str_right(Tensor offsets, Tensor bytes, int64_t n);
std::vector<Tensor> str_reverse(Tensor offsets, Tensor bytes);
std::vector<Tensor> str_normalize_ascii(Tensor offsets, Tensor bytes,
                                        OptTensor valid, bool remove_punct,
                                        bool lowercase, bool white_space);

// regex / LIKE by DFA tables (regex.hip).  table: int16 [n_states,
// n_classes], byte_class: uint8 [256], flags: uint8 [n_states] (1 matched,
// 2 matches at end of row, 4 dead); all three are staged in LDS.
Tensor regex_match(Tensor offsets, Tensor bytes, Tensor table,
                   Tensor byte_class, Tensor flags, int64_t n_classes,
                   int64_t start);
// match positions with `re.finditer` semantics (regex_dfa.py SpanProgram):
// a forward priority DFA finds each match end, a reverse DFA its start; flags
// are 1 (match) and 4 (dead).  regex_count: matches per row, 0 where `valid`
// is false, at most `limit` (-1: all).  regex_spans: {starts, ends}, absolute
// positions in `bytes`, row i's k-th match at match_offsets[i] + k.
Tensor regex_count(Tensor offsets, Tensor bytes, OptTensor valid,
                   Tensor fwd_table, Tensor byte_class, Tensor fwd_flags,
                   int64_t n_classes, int64_t start, int64_t limit);
std::vector<Tensor> regex_spans(Tensor offsets, Tensor bytes, OptTensor valid,
                                Tensor fwd_table, Tensor byte_class,
                                Tensor fwd_flags, int64_t n_classes,
                                int64_t start, Tensor rev_table,
                                Tensor rev_flags, int64_t rev_start,
                                Tensor match_offsets, int64_t limit);
