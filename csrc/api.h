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

// top-k candidate selection (topk.hip), an MSD radix select.
// keys: int64 [n] holding u64 order keys (unsigned compare), 1 <= k <= n.
// T = the k-th smallest key.  Returns {rows, stats}:
//   rows  int64 [m], ascending: every i with keys[i] <= T  (m >= k)
//   stats int64 [3]: {T as bit pattern, #keys < T, #keys == T}
// Checked on the host: dtype, contiguity, device, rank, 1 <= k <= n.
std::vector<Tensor> topk_candidates(Tensor keys, int64_t k);

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

// framed window aggregate (window.hip).  Sorted position p holds original row
// perm[p]; partition g owns sorted positions [seg_offsets[g],
// seg_offsets[g+1]).  values (float64 or int64; unused by a count) and valid
// are in original row order, and so are the outputs {value, count}: count is
// the number of non-null inputs in the row's frame (int64), value the
// aggregate over them, 0 where count is 0.  value is float64 for mean,
// variance (population) and stddev and for float64 input, else int64 and
// exact.  Bounds: kind 0 unbounded, 1 current row + offset, 2 (hi only, with
// lo unbounded) end of the row's peer run, read from new_peer, a bool per
// sorted position that is true where a new run of equal order keys starts.
// Checked on the host: dtype, contiguity, device, rank, lengths, op and
// bound codes.  The Python wrapper answers for what lives in device memory:
// perm a permutation, gids below seg_offsets.numel() - 1, monotone offsets
// from 0 to n that match the sort.
std::vector<Tensor> window_agg(
    OptTensor values, OptTensor valid, Tensor perm, Tensor gids,
    Tensor seg_offsets, OptTensor new_peer, int64_t lo_kind, int64_t lo_off,
    int64_t hi_kind, int64_t hi_off,
    int64_t op /*0 sum, 1 count, 2 mean, 3 min, 4 max, 5 variance, 6 stddev*/);

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
// Filter -> Aggregate in one JIT kernel.  `body` is the straight-line row
// code; ops[a] is the AggOp of accumulator a and own_valid[a] says whether
// its input can be null.  Returns {acc f64 [A*G], cnt i64 [A*G], hit i64 [G]},
// slot of (a, g) at a * G + g; hit counts the rows that pass per group.
// fused_agg_source is host-only: the full kernel text for that plan.
std::string fused_agg_source(const std::string& body,
                             std::vector<int64_t> col_has_valid,
                             std::vector<int64_t> ops,
                             std::vector<int64_t> own_valid, int64_t groups);
std::vector<Tensor> fused_agg_jit(const std::string& body,
                                  std::vector<Tensor> cols,
                                  std::vector<OptTensor> valids,
                                  std::vector<int64_t> ops,
                                  std::vector<int64_t> own_valid,
                                  int64_t groups, int64_t n);

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

// text <-> values (strparse.hip).  Each parse returns {values, status}:
// status uint8 [n] is 0 parsed, 1 null (`valid` false; for the numeric targets
// also the empty row), 2 "the host must decide"; values are 0 where status is
// not 0.  str_parse_int: [+-]?[0-9]+ in [lo, hi], int64.  str_parse_decimal:
// int64 scaled by 10^scale, |v| <= max_abs < 10^18, no exponent, no nonzero
// digit past `scale`.  str_parse_float: float64, correctly rounded or status
// 2; pow5 is int64 [651, 2], the {low, high} words of the 128-bit powers of
// five for 10^-342 .. 10^308.  str_parse_datetime: sep 0 reads YYYY-MM-DD as
// int32 days since 1970-01-01, sep ' ' or 'T' reads YYYY-MM-DD<sep>HH:MM:SS
// as int64 microseconds.  format_int (int64) and format_date (int32 days in
// years 0001-9999) return {offsets, bytes}; null rows are empty.
// strparse_staging switches the LDS staging of the parse kernels on or off
// and returns the previous setting.
std::vector<Tensor> str_parse_int(Tensor offsets, Tensor bytes, OptTensor valid,
                                  int64_t lo, int64_t hi);
std::vector<Tensor> str_parse_decimal(Tensor offsets, Tensor bytes,
                                      OptTensor valid, int64_t scale,
                                      int64_t max_abs);
std::vector<Tensor> str_parse_float(Tensor offsets, Tensor bytes,
                                    OptTensor valid, Tensor pow5);
std::vector<Tensor> str_parse_datetime(Tensor offsets, Tensor bytes,
                                       OptTensor valid, int64_t sep);
std::vector<Tensor> format_int(Tensor values, OptTensor valid);
std::vector<Tensor> format_date(Tensor days, OptTensor valid);
bool strparse_staging(bool on);

// CSV structure of one chunk (csv.hip): `data` uint8 [n], n < 2^31, 16-byte
// aligned, beginning at a record start.  csv_structure returns {sepmask int16
// [ceil(n / 4096) * 256] (bit i of entry k: byte 16 k + i is a delim or '\n'
// outside quotes), tile_base int32 [ceil(n / 4096)] (separators before each
// 4096-byte tile), info int32 [8]}.  info: [0] error bits (1 irregular quote,
// 2 invalid UTF-8, 4 ragged, 8 blank line, 16 a '\r' outside quotes that no
// '\n' follows), [1] UTF-8 continuation bytes claimed minus present (0 in a
// valid chunk), [2] position of the last '\n' separator + 1, [3] the
// separator count S, [4] 1 when the chunk ends inside quotes.  csv_emit
// returns sep_pos int32 [S] in byte order and fills info[2] and the ragged
// and blank-line bits for records of `ncols` fields.  csv_field_lens
// returns {seg_start int64 [nsel, nrows], lens int64 [nsel, nrows], any_quoted
// int32 [nsel]} for rows [row0, row0 + nrows) of the columns `cols`: where a
// field's content starts in `data`, its length once outer quotes are dropped
// and "" is read as one quote, and whether any field of the column is quoted.
// csv_extract writes one column's bytes for offsets out_offsets int64
// [nrows + 1] ending in `total`; `quoted` is the column's any_quoted.
// csv_precheck turns status 0 into 2 where pyarrow's CSV converters differ
// from str_parse_*: kind 0 signed integer (leading '+'), 1 unsigned integer
// (leading '+' or '-'), 2 decimal (more fractional digits than `scale`).
std::vector<Tensor> csv_structure(Tensor data, int64_t delim);
Tensor csv_emit(Tensor data, Tensor sepmask, Tensor tile_base, Tensor info,
                int64_t S, int64_t ncols);
std::vector<Tensor> csv_field_lens(Tensor data, Tensor sep_pos, int64_t ncols,
                                   int64_t row0, int64_t nrows,
                                   std::vector<int64_t> cols);
Tensor csv_extract(Tensor data, Tensor sep_pos, int64_t ncols, int64_t row0,
                   int64_t col, Tensor seg_start, Tensor out_offsets,
                   int64_t total, bool quoted);
void csv_precheck(Tensor offsets, Tensor bytes, Tensor status, int64_t kind,
                  int64_t scale);

// JSON-lines structure of one chunk (json.hip): `data` uint8 [n], n < 2^31,
// 16-byte aligned, beginning at a record start.  json_structure returns
// {structmask int16 [ceil(n / 4096) * 256] (bit i of entry k: byte 16 k + i
// is one of { } [ ] : , '\n' outside strings), depth_in, tok_base, close_base
// int32 [ceil(n / 4096)] (nesting depth, tokens and record ends before each
// tile), info int32 [8]}.  info: [0] error bits (1 irregular, 2 invalid UTF-8,
// 4 a run of 64 or more '\', 8 depth below 0 or a line end inside a record,
// 16 a key with a backslash, 32 a key outside the names, 64 a key twice in a
// record, 128 a bad escape or lone surrogate, 256 a raw byte < 0x20 in a
// string), [1] UTF-8 continuation bytes claimed minus present, [2] one past
// the last '\n' at depth 0 (consumed), [3] the token count T, [4] 1 when the
// chunk ends inside a string, [5] the longest record's bytes, [6] the records
// before `consumed`, [7] the record ends R of the whole chunk.  json_tokens
// returns int32 [2, T] in byte order: positions, and row << 2 | kind with
// kind 0 a record's '{', 1 a depth-1 ':', 2 a depth-1 ',', 3 the record's
// '}'.  json_keys packs 1..256 names of at most 2048 bytes (hash table,
// offsets, bytes) into a host int32 tensor for the LDS of json_fields, which
// checks the tokens before `consumed`, fills info[6] and returns {field_tok
// int32 [ncols, R] (the ':' token of each name per row, -1 where absent),
// row_end int32 [R]}.  json_values returns, for the first `nrows` rows,
// {kinds uint8 [ncols, nrows] (0 null or absent, 1 false, 2 true, 3 number,
// 4 string, 5 nested), raw_start, raw_len int64 [ncols, nrows] (the trimmed
// value text, a string's with its quotes), ulen int64 [ncols, nrows] (a
// string's unescaped length), seen int32 [ncols] (bit k: kind k occurs; 256:
// a string holds a backslash)} and fills info[5].  json_extract writes one
// column's bytes for out_offsets int64 [nrows + 1] ending in `total`:
// without `unescape` a segment copy from raw_start, else the content of the
// kind-4 rows with their escapes decoded.
Tensor json_keys(std::vector<std::string> names);
std::vector<Tensor> json_structure(Tensor data);
Tensor json_tokens(Tensor data, Tensor structmask, Tensor depth_in,
                   Tensor tok_base, Tensor close_base, int64_t T);
std::vector<Tensor> json_fields(Tensor data, Tensor tokens, int64_t consumed,
                                int64_t R, Tensor keys, int64_t ncols,
                                Tensor info);
std::vector<Tensor> json_values(Tensor data, Tensor tokens, Tensor field_tok,
                                Tensor row_end, int64_t nrows, Tensor info);
Tensor json_extract(Tensor data, Tensor kinds, Tensor raw_start,
                    Tensor raw_len, Tensor out_offsets, int64_t total,
                    bool unescape);

// Parquet page decode (parquet.hip).  `buf` uint8, 16-byte aligned, holds a
// row group's uploaded column-chunk bytes and the decompression arena behind
// them; `desc` int64 [pages, 12] is the page table laid out at the top of
// parquet.hip; `status` int32 [pages] collects 1 (a descriptor outside `buf`
// or the outputs) and 2 (malformed page content) and is never cleared here.
// pq_snappy decompresses every row with src_len > 0 in place.  pq_levels
// decodes definition levels of width 1 for `nrows` rows -> {validity bool
// [nrows], map int32 [nrows] (map[first_row + j]: the row of the page's j-th
// stored value), stored int32 [pages]}.  pq_plain writes the PLAIN pages and
// pq_rle_values the dictionary-index and RLE-boolean pages of `desc` into
// `out`, uint8 viewed as rows of out_width bytes; rows of other pages and
// null rows are left as they are.  map and stored come from pq_levels, or
// are both absent for a column without nulls.  in_width is the stored width:
// 0 for booleans (bits), 4 or 8 little-endian, or 1..8 big-endian bytes.
// dict holds dict_n values of out_width bytes; without it the index itself
// is stored, and must be < dict_n.  pq_dict_strings decodes the one
// dictionary page `desc` [1, 12] of n PLAIN BYTE_ARRAY values with `total`
// bytes -> {offsets int64 [n + 1], bytes uint8 [total]}.
void pq_snappy(Tensor buf, Tensor desc, Tensor status);
std::vector<Tensor> pq_levels(Tensor buf, Tensor desc, int64_t nrows,
                              Tensor status);
void pq_plain(Tensor buf, Tensor desc, OptTensor map, OptTensor stored,
              Tensor out, int64_t in_width, bool big_endian,
              int64_t out_width, Tensor status);
void pq_rle_values(Tensor buf, Tensor desc, OptTensor map, OptTensor stored,
                   OptTensor dict, int64_t dict_n, Tensor out,
                   int64_t out_width, Tensor status);
std::vector<Tensor> pq_dict_strings(Tensor buf, Tensor desc, int64_t n,
                                    int64_t total, Tensor status);
