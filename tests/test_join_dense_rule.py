"""Which joins take the direct-address path (rowops._dense_eligible)."""
import pytest

from daft_amd.kernels import rowops
from daft_amd.schema import DataType
from daft_amd.series import Series

F = rowops._DENSE_PROBE_FACTOR
LIMIT = rowops._DENSE_JOIN_LIMIT


@pytest.mark.parametrize("n_l, n_r, rng, want", [
    # admitted by the build side: up to 16x sparse, or small outright
    (400, 150, 200, True),
    (1, 1000, 16 * 1000, True),
    (1, 1, 1 << 20, True),
    (1, 1, (1 << 20) + 1, False),
    (1, 100_000, 16 * 100_000, True),
    (1, 100_000, 16 * 100_000 + 1, False),
    # admitted by the probe side: a table proportional to the probe
    (600_000_000, 16_800, 20_000_000, True),      # q17's shape
    (10_000_000, 2, F * 10_000_000, True),
    (10_000_000, 2, F * 10_000_000 + 1, False),
    # pinned by test_dataframe: build keys [1, 10**9], 400 probe rows
    (400, 2, 10**9, False),
    # pinned by test_dataframe: build keys [1, 2, 2]; the rule admits the
    # range, the duplicate check in the build then refuses the inner join
    (400, 3, 2, True),
    # the table cap holds whatever the sizes
    (1 << 40, 1 << 30, LIMIT, True),
    (1 << 40, 1 << 30, LIMIT + 1, False),
    (400, 150, 0, False),
    (400, 150, -5, False),
])
def test_dense_eligible(n_l, n_r, rng, want):
    assert rowops._dense_eligible(n_l, n_r, rng) is want


def test_pinned_cases_still_fall_back():
    lk = [Series.from_pylist("k", list(range(50, 450)), DataType.int64())]
    for build in ([1, 10**9], [1, 2, 2]):
        rk = [Series.from_pylist("k", build, DataType.int64())]
        assert rowops._dense_key_join(lk, rk, "inner") is None
