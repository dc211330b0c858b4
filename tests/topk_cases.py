"""Top-k test keys: name -> (keys, descending, nulls_first), host, read-only."""
import functools

import numpy as np
import torch

from daft_amd.schema import DataType
from daft_amd.series import Series

KS = (1, 2, 7, 50)


def _int64(rng, n, lo, hi, nulls=True):
    valid = torch.from_numpy(rng.random(n) > 0.15) if nulls else None
    return Series("i", DataType.int64(), validity=valid,
                  data=torch.from_numpy(rng.integers(lo, hi, size=n)))


@functools.lru_cache(maxsize=None)
def key_lists(n):
    rng = np.random.default_rng(n)
    cases = {}
    ints = _int64(rng, n, -40, 40)
    for desc in (False, True):
        for nf in (False, True):
            cases[f"int64_desc{int(desc)}_nf{int(nf)}"] = ([ints], [desc], [nf])
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, -1.5])
    cases["float64_special_desc"] = ([Series(
        "f", DataType.float64(), data=torch.from_numpy(
            special[rng.integers(0, 7, size=n)]))], [True], [False])
    revenue = Series("r", DataType.float64(),
                     data=torch.from_numpy(rng.integers(0, 25, size=n) / 4.0))
    date = Series("d", DataType.date(), data=torch.from_numpy(
        rng.integers(9000, 9040, size=n).astype(np.int32)))
    cases["q3_float_desc_date_asc"] = ([revenue, date], [True, False],
                                       [False, False])
    # equal in the first 8 bytes, so the image ties and the tail decides
    words = [None if v % 11 == 0 else f"customer#{v % 37:04d}"
             for v in rng.integers(0, 1000, size=n)]
    cases["string_long_prefix_then_int"] = (
        [Series.from_pylist("s", words, DataType.string()),
         _int64(rng, n, 0, 5)], [False, True], [True, False])
    vocab = Series.from_pylist("v", ["pear", "apple", "fig", "kiwi", "date"],
                               DataType.string())
    cases["dict_string"] = ([Series.make_dict(
        "ds", vocab, torch.from_numpy(rng.integers(0, 5, size=n)),
        validity=torch.from_numpy(rng.random(n) > 0.1))], [True], [False])
    flag = torch.from_numpy(rng.random(n) > 0.5)
    cases["bool_then_int"] = ([Series("b", DataType.bool(), data=flag),
                               _int64(rng, n, 0, 1000, nulls=False)],
                              [False, False], [False, False])
    edge = np.array([-2 ** 63, 2 ** 63 - 1, 0, 5])[rng.integers(0, 4, size=n)]
    sentinel = Series("e", DataType.int64(), data=torch.from_numpy(edge),
                      validity=torch.from_numpy(rng.random(n) > 0.3))
    for nf in (False, True):     # int64 min / max are the null images
        cases[f"valid_on_null_sentinel_nf{int(nf)}"] = ([sentinel], [False],
                                                        [nf])
    return cases


CASE_NAMES = tuple(key_lists(8))
