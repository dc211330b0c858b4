"""Top-k pruning on the host (numpy stand-in for the radix select): the image
and candidate sort of rowops._topk_select must equal argsort_multi(...)[:k]."""
import pytest
import torch

from daft_amd.kernels import rowops

import topk_cases as tc

N = 300


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_topk_select_equals_full_sort_prefix(name):
    keys, desc, nf = tc.key_lists(N)[name]
    full = rowops.argsort_multi(keys, desc, nf)
    for k in tc.KS + (N - 1, N):
        got = rowops._topk_select(keys, desc, nf, k)
        assert torch.equal(got, full[:k]), (name, k)
        assert torch.equal(rowops.topk_multi(keys, desc, nf, k), full[:k])
