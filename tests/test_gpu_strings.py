"""HIP string kernels (csrc/strings.hip, the string-sort key in
csrc/sort.hip, take_string / merge_strings in csrc/kernels.hip) against the
Python oracle in strings_cases.py: multi-byte UTF-8, sizes that cross the
256-thread block edge in rows and in output bytes, sliced, dictionary and
null-over-bytes columns.  All comparisons are exact.

The wrapper tests run the same matrix as test_strings_parity.py on cuda:0;
the raw-binding tests call the extension directly.  Every binding checks
its tensors on the host before it launches anything (csrc/host_args.h): a
column whose offsets are not contiguous int64 [n + 1] on the GPU or whose
bytes are not contiguous uint8 on the same device, columns of different
length, and a pattern, mask or index of the wrong dtype or device raise
RuntimeError; the refusal tests at the end pin that down.  Values in device
memory are not checked: the raw bindings are never given a zero-length LIKE
needle, offsets that decrease or point past the bytes, or an index out of
range; the wrappers filter those out and the kernels do not guard against
them.  A negative start is refused by str_substr itself."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from daft_amd import DataType, Series
from daft_amd.kernels import native_required

import strings_cases as sc

DEV = "cuda:0"
MATRIX = [(n, v) for n in sc.SIZES for v in sc.VARIANTS]
matrix = pytest.mark.parametrize("n,variant", MATRIX)
RAW_SIZES = [257, 4099]
raw_sizes = pytest.mark.parametrize("n", RAW_SIZES)


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    # the HIP extension must be present on a GPU box — no silent fallback
    native_required()


# ---------------------------------------------------------------------------
# wrappers: daft_amd/kernels/strings.py on cuda:0 Series
# ---------------------------------------------------------------------------

def test_columns_are_on_the_device():
    for variant in sc.VARIANTS:
        s, vals = sc.column(257, variant, DEV)
        assert s.is_gpu()
        assert s.to_pylist() == list(vals)
    s, _ = sc.column(257, "slice", DEV)
    assert s.data.storage_offset() > 0


@matrix
def test_find_family(n, variant):
    sc.check_find_family(n, variant, DEV)


@matrix
def test_like(n, variant):
    sc.check_like(n, variant, DEV)


@matrix
def test_lengths(n, variant):
    sc.check_lengths(n, variant, DEV)


@matrix
def test_substr_left(n, variant):
    sc.check_substr(n, variant, DEV)


def test_substr_binary_counts_bytes():
    sc.check_substr_binary(DEV)


def test_substr_rejects_negative():
    sc.check_substr_rejects_negative(DEV)


@matrix
def test_lower_upper(n, variant):
    sc.check_case(n, variant, DEV)


@raw_sizes
def test_lower_upper_ascii_kernel(n):
    sc.check_case_ascii(n, DEV)


@matrix
def test_concat(n, variant):
    sc.check_concat(n, variant, DEV)


@matrix
def test_compare(n, variant):
    sc.check_compare(n, variant, DEV)


# ---------------------------------------------------------------------------
# raw bindings
# ---------------------------------------------------------------------------

def _raw(n):
    """Plain device column with no validity: nulls become empty rows."""
    vals = ["" if v is None else v for v in sc.corpus(n)]
    s = Series.from_pylist("s", vals, DataType.string(), device=DEV)
    return s, vals


def _pat(p: str) -> torch.Tensor:
    return torch.tensor(list(p.encode()), dtype=torch.uint8, device=DEV)


def _o_find_mode(vals, p, mode):
    if mode == 0:
        return sc.o_find(vals, p)
    f = sc.o_startswith if mode == 1 else sc.o_endswith
    return [0 if hit else -1 for hit in f(vals, p)]


def _strings_of(off, data):
    off = off.cpu().numpy()
    buf = data.cpu().numpy().tobytes()
    assert off[0] == 0 and off[-1] == len(buf)
    return [buf[off[i]:off[i + 1]] for i in range(len(off) - 1)]


@raw_sizes
def test_raw_str_find(n):
    nat = native_required()
    s, vals = _raw(n)
    whole_row = next(v for v in vals if len(v) > 8 and not v.isascii())
    for p in sc.NEEDLES[1:] + [whole_row]:
        for mode in (0, 1, 2):
            out = nat.str_find(s.offsets, s.data, _pat(p), mode)
            assert out.cpu().tolist() == _o_find_mode(vals, p, mode), \
                (p, mode)
    assert sc.o_find(vals, whole_row).count(0) >= 1


def test_raw_str_find_edges():
    """Match ending on the last byte, restart after a partial match, a
    pattern longer than the row, and rows that touch their neighbours."""
    nat = native_required()
    vals = ["xxab", "ab", "aab", "abx", "a", "", "aaab", "abab", "aabaab",
            "b", "xa", "ab", "€a", "x€a", "€", "€b", "aa"]
    s = Series.from_pylist("s", vals, DataType.string(), device=DEV)
    for p in ("ab", "aab", "b", "€a", "aabaab", "aabaabx"):
        for mode in (0, 1, 2):
            out = nat.str_find(s.offsets, s.data, _pat(p), mode)
            assert out.cpu().tolist() == _o_find_mode(vals, p, mode), \
                (p, mode)
    assert sc.o_find(vals, "ab")[:4] == [2, 0, 1, 0]
    assert sc.o_find(vals, "aab")[6] == 1        # "aaab": restart after "aa"


@raw_sizes
def test_raw_str_like(n):
    nat = native_required()
    s, vals = _raw(n)
    ran = 0
    for pat in sc.LIKE_PATTERNS:
        parts = pat.split("%")
        needles = [p.encode() for p in parts if p]
        if "_" in pat or len(parts) == 1 or not needles:
            continue
        assert all(len(nd) > 0 for nd in needles)
        lens = torch.tensor([len(nd) for nd in needles], dtype=torch.int64,
                            device=DEV)
        blob = torch.tensor(list(b"".join(needles)), dtype=torch.uint8,
                            device=DEV)
        out = nat.str_like(s.offsets, s.data, blob, lens, bool(parts[0]),
                           bool(parts[-1]))
        assert out.cpu().tolist() == sc.o_like(vals, pat), pat
        ran += 1
    assert ran == 8


def test_raw_str_like_anchor_overlap():
    """An anchored prefix and suffix must not share bytes, and needles
    match left to right without overlapping."""
    nat = native_required()
    vals = ["a", "aa", "aba", "ab", "abab", "ababab", "aab", "abaab", "",
            "é😀", "😀é", "é😀é", "xabxab"]
    s = Series.from_pylist("s", vals, DataType.string(), device=DEV)
    for pat in ("a%a", "ab%ab", "%ab%ab%", "aba%aba", "%é%😀%", "é%é"):
        parts = pat.split("%")
        needles = [p.encode() for p in parts if p]
        lens = torch.tensor([len(nd) for nd in needles], dtype=torch.int64,
                            device=DEV)
        blob = torch.tensor(list(b"".join(needles)), dtype=torch.uint8,
                            device=DEV)
        out = nat.str_like(s.offsets, s.data, blob, lens, bool(parts[0]),
                           bool(parts[-1]))
        assert out.cpu().tolist() == sc.o_like(vals, pat), pat
    assert sc.o_like(vals, "a%a")[:3] == [False, True, True]
    assert sc.o_like(vals, "aba%aba")[2] is False


@raw_sizes
def test_raw_str_substr(n):
    nat = native_required()
    s, vals = _raw(n)
    for start, length in sc.SUBSTR_ARGS:
        assert start >= 0
        ln = -1 if length is None else length
        off, data = nat.str_substr(s.offsets, s.data, start, ln, True)
        want = [v.encode() for v in sc.o_substr(vals, start, length)]
        assert _strings_of(off, data) == want, (start, length)
        # BINARY columns slice bytes
        off, data = nat.str_substr(s.offsets, s.data, start, ln, False)
        want = sc.o_substr([v.encode() for v in vals], start, length)
        assert _strings_of(off, data) == want, (start, length)


@raw_sizes
def test_raw_str_concat(n):
    nat = native_required()
    s, vals = _raw(n)
    vals2 = sc.shuffled(vals)
    s2 = Series.from_pylist("t", vals2, DataType.string(), device=DEV)
    lit = Series.from_pylist("l", ["€-"], DataType.string(),
                             device=DEV).broadcast(n)
    cols = [(s, vals), (lit, ["€-"] * n), (s2, vals2)]
    for k in (1, 2, 3):
        off, data = nat.str_concat([c.offsets for c, _ in cols[:k]],
                                   [c.data for c, _ in cols[:k]])
        want = [v.encode() for v in sc.o_concat(*[v for _, v in cols[:k]])]
        assert _strings_of(off, data) == want


@raw_sizes
def test_raw_str_char_length(n):
    s, vals = _raw(n)
    out = native_required().str_char_length(s.offsets, s.data)
    assert out.cpu().tolist() == sc.o_length(vals)


@raw_sizes
def test_raw_string_compare(n):
    s, vals = _raw(n)
    vals2 = sc.shuffled(vals)
    for i in range(0, n, 5):
        vals2[i] = vals[i]
    for i in range(1, n, 5):
        vals2[i] = vals[i][:-1]
    s2 = Series.from_pylist("t", vals2, DataType.string(), device=DEV)
    out = native_required().string_compare(s.offsets, s.data, s2.offsets,
                                           s2.data)
    want = sc.o_compare3(vals, vals2)
    assert out.cpu().tolist() == want
    assert {-1, 0, 1} == set(want)


@raw_sizes
def test_raw_string_chunk_key(n):
    s, vals = _raw(n)
    assert max(len(v.encode()) for v in vals) > 40
    for chunk in range(6):
        out = native_required().string_chunk_key(s.offsets, s.data, chunk)
        got = out.cpu().numpy().view(np.uint64).tolist()
        assert got == sc.o_chunk_key(vals, chunk), chunk


@pytest.mark.parametrize("variant", ["plain", "slice", "masked"])
@raw_sizes
def test_take_string(n, variant):
    s, vals = sc.column(n, variant, DEV)
    m = len(vals)
    rng = random.Random(3)
    idx = [rng.randrange(m) for _ in range(m + 300)]     # with repeats
    for i in range(0, len(idx), 11):
        idx[i] = -1
    out = s.take(torch.tensor(idx, dtype=torch.int64, device=DEV))
    sc.assert_strings(out, [None if i < 0 else vals[i] for i in idx])
    # the binding itself, on clamped indices
    safe = [max(i, 0) for i in idx]
    off, data = native_required().take_string(
        s.offsets, s.data, torch.tensor(safe, dtype=torch.int64, device=DEV))
    under = _strings_of(s.offsets, s.data)
    assert _strings_of(off, data) == [under[i] for i in safe]


@matrix
def test_if_else_merge_strings(n, variant):
    sc.check_if_else(n, variant, DEV)


# ---------------------------------------------------------------------------
# sort
# ---------------------------------------------------------------------------

@matrix
def test_sort(n, variant):
    sc.check_sort(n, variant, DEV)


def test_sort_long_shared_chunks():
    sc.check_sort_long(DEV)


def test_sort_nul_tail():
    sc.check_sort_nul_tail(DEV)


@pytest.mark.parametrize("byte_positions", [(3,), (0, 7)])
def test_radix_argsort_skips_constant_bytes(byte_positions):
    """Keys that vary in one or two byte positions only: every other pass
    of the 8 sees a single digit and is skipped."""
    rng = np.random.default_rng(7)
    n = 4099
    keys = np.full(n, 0x5A11223344556677, dtype=np.uint64)
    for b in byte_positions:
        shift = np.uint64(8 * b)
        keys &= ~(np.uint64(0xFF) << shift)
        keys |= rng.integers(0, 256, n).astype(np.uint64) << shift
    want = np.argsort(keys, kind="stable")
    t = torch.from_numpy(keys.view(np.int64)).to(DEV)
    got = native_required().radix_argsort(t).cpu().numpy()
    assert (got == want).all()
    assert len(np.unique(keys)) < n          # ties: stability is checked


# ---------------------------------------------------------------------------
# refusals: a bad argument raises on the host, before anything is launched;
# the valid call after each group shows that the context is still sound
# ---------------------------------------------------------------------------

def _col3():
    s = Series.from_pylist("s", sc.REFUSED_VALUES, DataType.string(),
                           device=DEV)
    return s.offsets, s.data


def _col4():
    vals = sc.REFUSED_VALUES + ["d"]
    s = Series.from_pylist("t", vals, DataType.string(), device=DEV)
    return s.offsets, s.data, vals


def test_str_find_refuses_bad_arguments():
    nat, vals = native_required(), sc.REFUSED_VALUES
    off, data = _col3()
    sc.assert_refuses_bad_columns(
        "str_find", lambda o, d: nat.str_find(o, d, _pat("b"), 0), off, data)
    with pytest.raises(RuntimeError, match="str_find: "):
        nat.str_find(off, data, _pat("b").cpu(), 0)
    with pytest.raises(RuntimeError, match="str_find: "):
        nat.str_find(off, data, _pat("abab")[::2], 0)
    assert nat.str_find(off, data, _pat("b"), 0).cpu().tolist() == \
        sc.o_find(vals, "b") == [1, -1, 1]


def test_str_like_refuses_bad_arguments():
    nat, vals = native_required(), sc.REFUSED_VALUES
    off, data = _col3()
    lens = torch.tensor([1, 1], dtype=torch.int64, device=DEV)

    def call(o, d, blob=_pat("ac"), lens=lens):
        return nat.str_like(o, d, blob, lens, True, True)
    sc.assert_refuses_bad_columns("str_like", call, off, data)
    with pytest.raises(RuntimeError, match="str_like: "):
        call(off, data, blob=_pat("ac").cpu())
    with pytest.raises(RuntimeError, match="str_like: "):
        call(off, data, lens=lens.to(torch.int32))
    with pytest.raises(RuntimeError, match="str_like: "):
        call(off, data, lens=lens.cpu())
    assert call(off, data).cpu().tolist() == sc.o_like(vals, "a%c") == \
        [False, False, True]


def test_str_case_refuses_bad_arguments():
    nat, vals = native_required(), sc.REFUSED_VALUES
    off, data = _col3()
    sc.assert_refuses_bad_columns(
        "str_case", lambda o, d: nat.str_case(o, d, 1), off, data)
    assert _strings_of(off, nat.str_case(off, data, 1)) == \
        [v.encode() for v in sc.o_upper(vals)]


def test_str_substr_refuses_bad_arguments():
    nat, vals = native_required(), sc.REFUSED_VALUES
    off, data = _col3()
    sc.assert_refuses_bad_columns(
        "str_substr", lambda o, d: nat.str_substr(o, d, 1, 1, True), off,
        data)
    assert _strings_of(*nat.str_substr(off, data, 1, 1, True)) == \
        [v.encode() for v in sc.o_substr(vals, 1, 1)] == [b"b", b"", b"b"]


def test_str_concat_refuses_bad_arguments():
    nat, vals = native_required(), sc.REFUSED_VALUES
    off, data = _col3()
    off4, data4, _ = _col4()
    for slot in (0, 1):       # the bad column first, and after a good one

        def call(o, d):
            offs, datas = [off, off], [data, data]
            offs[slot], datas[slot] = o, d
            return nat.str_concat(offs, datas)
        sc.assert_refuses_bad_columns("str_concat", call, off, data)
    with pytest.raises(RuntimeError, match="str_concat: "):
        nat.str_concat([off, off4], [data, data4])
    with pytest.raises(RuntimeError, match="str_concat: "):
        nat.str_concat([off4, off], [data4, data])
    with pytest.raises(RuntimeError, match="str_concat: "):
        nat.str_concat([], [])
    with pytest.raises(RuntimeError, match="str_concat: "):
        nat.str_concat([off, off], [data])
    assert _strings_of(*nat.str_concat([off, off], [data, data])) == \
        [v.encode() for v in sc.o_concat(vals, vals)]


def test_str_char_length_refuses_bad_arguments():
    nat, vals = native_required(), sc.REFUSED_VALUES
    off, data = _col3()
    sc.assert_refuses_bad_columns("str_char_length", nat.str_char_length,
                                  off, data)
    assert nat.str_char_length(off, data).cpu().tolist() == \
        sc.o_length(vals) == [2, 1, 3]


def test_string_compare_refuses_bad_arguments():
    nat, vals = native_required(), sc.REFUSED_VALUES
    off, data = _col3()
    off4, data4, _ = _col4()
    sc.assert_refuses_bad_columns(
        "string_compare", lambda o, d: nat.string_compare(o, d, off, data),
        off, data)
    sc.assert_refuses_bad_columns(
        "string_compare", lambda o, d: nat.string_compare(off, data, o, d),
        off, data)
    with pytest.raises(RuntimeError, match="string_compare: "):
        nat.string_compare(off, data, off4, data4)
    with pytest.raises(RuntimeError, match="string_compare: "):
        nat.string_compare(off4, data4, off, data)
    other = ["ab", "a", "abd"]
    s2 = Series.from_pylist("t", other, DataType.string(), device=DEV)
    assert nat.string_compare(off, data, s2.offsets, s2.data).cpu() \
        .tolist() == sc.o_compare3(vals, other) == [0, 1, -1]


def test_string_chunk_key_refuses_bad_arguments():
    nat, vals = native_required(), sc.REFUSED_VALUES
    off, data = _col3()
    sc.assert_refuses_bad_columns(
        "string_chunk_key", lambda o, d: nat.string_chunk_key(o, d, 0), off,
        data)
    got = nat.string_chunk_key(off, data, 0).cpu().numpy().view(np.uint64)
    assert got.tolist() == sc.o_chunk_key(vals, 0)


def test_take_string_refuses_bad_arguments():
    nat = native_required()
    off, data = _col3()
    idx = torch.tensor([2, 0, 0, 1], dtype=torch.int64, device=DEV)
    sc.assert_refuses_bad_columns(
        "take_string", lambda o, d: nat.take_string(o, d, idx), off, data)
    for bad in (idx.cpu(), idx.to(torch.int32), idx[::2]):
        with pytest.raises(RuntimeError, match="take_string: "):
            nat.take_string(off, data, bad)
    under = [v.encode() for v in sc.REFUSED_VALUES]
    assert _strings_of(*nat.take_string(off, data, idx)) == \
        [under[i] for i in idx.cpu().tolist()]


def test_merge_strings_refuses_bad_arguments():
    nat, t_vals = native_required(), sc.REFUSED_VALUES
    t_off, t_data = _col3()
    f_vals = ["xyz", "", "é"]
    f = Series.from_pylist("f", f_vals, DataType.string(), device=DEV)
    f_off, f_data = f.offsets, f.data
    off4, data4, _ = _col4()
    mask = torch.tensor([True, False, False], device=DEV)
    want = [(t if m else v).encode()
            for m, t, v in zip(mask.cpu().tolist(), t_vals, f_vals)]
    out_off = torch.tensor(np.cumsum([0] + [len(w) for w in want]),
                           dtype=torch.int64, device=DEV)
    sc.assert_refuses_bad_columns(
        "merge_strings",
        lambda o, d: nat.merge_strings(mask, o, d, f_off, f_data, out_off),
        t_off, t_data)
    sc.assert_refuses_bad_columns(
        "merge_strings",
        lambda o, d: nat.merge_strings(mask, t_off, t_data, o, d, out_off),
        f_off, f_data)
    mask4 = torch.tensor([True, False, False, True], device=DEV)
    out_off4 = torch.cat([out_off, out_off[-1:]])
    for args in ((mask, t_off, t_data, off4, data4, out_off),
                 (mask, off4, data4, f_off, f_data, out_off),
                 (mask4, t_off, t_data, f_off, f_data, out_off),
                 (mask, t_off, t_data, f_off, f_data, out_off4),
                 (mask.cpu(), t_off, t_data, f_off, f_data, out_off),
                 (mask.to(torch.uint8), t_off, t_data, f_off, f_data,
                  out_off),
                 (mask, t_off, t_data, f_off, f_data,
                  out_off.to(torch.int32)),
                 (mask, t_off, t_data, f_off, f_data, out_off.cpu())):
        with pytest.raises(RuntimeError, match="merge_strings: "):
            nat.merge_strings(*args)
    out = nat.merge_strings(mask, t_off, t_data, f_off, f_data, out_off)
    assert _strings_of(out_off, out) == want == [b"ab", b"", "é".encode()]


# ---------------------------------------------------------------------------
# str_substr through the ragged copy it shares with copy_segments, at the
# shapes where the per-byte search for the output row can go wrong
# ---------------------------------------------------------------------------

def _substr_rows(name):
    """(values, start, length) of one shape."""
    if name == "all_empty":          # total == 0: nothing is launched
        return ["ab", "", "€", "abcd"], 5, None
    if name == "empty_runs":
        # 300 rows: the first 5 and last 5 results are empty (rows shorter
        # than start), and so are runs of 1, 2, .. rows in between
        vals, gap, run = [], 0, 1
        for i in range(290):
            if gap == 0:
                vals += [""] * run
                gap, run = 7, run % 6 + 1
            else:
                vals.append("é" * 2 + sc.ALPHABET[i % 11] * (1 + i % 9))
                gap -= 1
        vals = ["", "a", "é", "ab", "b"] + vals[:290] + ["é", "", "ab", "a",
                                                           ""]
        return vals, 2, 5
    if name == "one_long_row":       # 600 bytes out: two block edges
        return ["x" + "ab€" * 120], 1, None
    assert name == "one_row"
    return ["a€b"], 1, 1


@pytest.mark.parametrize("by_char", [True, False])
@pytest.mark.parametrize("name", ["all_empty", "empty_runs", "one_long_row",
                                  "one_row"])
def test_str_substr_row_search(name, by_char):
    vals, start, length = _substr_rows(name)
    s = Series.from_pylist("s", vals, DataType.string(), device=DEV)
    src = vals if by_char else [v.encode() for v in vals]
    want = [v.encode() if by_char else v
            for v in sc.o_substr(src, start, length)]
    off, data = native_required().str_substr(
        s.offsets, s.data, start, -1 if length is None else length, by_char)
    assert _strings_of(off, data) == want
    sizes = [len(w) for w in want]
    if name == "all_empty":
        assert sum(sizes) == 0
    elif name == "empty_runs":
        assert len(vals) == 300 and not any(sizes[:5] + sizes[-5:])
        assert any(sizes[i] == sizes[i + 1] == 0 < sizes[i + 2]
                   for i in range(5, 290))
    elif name == "one_long_row":
        assert sizes == [600]
