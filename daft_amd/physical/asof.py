"""As-of join: for each left row, the one right row whose `on` key is
closest under the strategy, among the right rows with equal `by` keys.

    backward  greatest right key <= left key (< when not allow_exact);
              among equal right keys the highest original row
    forward   least right key >= left key (> when not allow_exact);
              among equal right keys the lowest original row
    nearest   the nearer of the forward pick and the strict backward pick
              (the neighbours of the left key); a tie goes to the forward
              one, the larger key

A row is usable when its on-key and every `by` key are valid; an unusable
row never matches.  Keys are compared as the order-preserving u64 patterns of
rowops._order_key_u64, so NaN == NaN above +inf and -0.0 == +0.0.

Layout handed to the probe: the usable right rows stably sorted by
(group id, key), `seg_offsets[g]..seg_offsets[g + 1]` the sorted positions
of group g, `right_rows` the original row of each sorted position, and one
group id per left row (-1 = matches nothing).  Group ids and the sort run on
the existing group-by and radix kernels; the probe is csrc/asof.hip on the
device and one vectorised numpy search on the host.  Nothing loops over
groups or rows, and the number of host syncs does not depend on either."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from ..kernels import native_required, rowops
from ..logical.plan import ASOF_STRATEGIES, asof_key_supported
from ..recordbatch import RecordBatch
from ..series import Series
from ..schema import DataType

_SIGN64 = -(1 << 63)


def _check_strategy(strategy: str, allow_exact: bool) -> int:
    if strategy not in ASOF_STRATEGIES:
        raise ValueError(f"join_asof: strategy must be one of "
                         f"{ASOF_STRATEGIES}, got {strategy!r}")
    if strategy == "nearest" and not allow_exact:
        raise ValueError("join_asof: nearest cannot exclude exact matches")
    return ASOF_STRATEGIES.index(strategy)


def _common_keys(left: Series, right: Series) -> Tuple[Series, Series]:
    """Both on-keys in one dtype: unchanged when they agree, float64 when
    either is floating, int64 otherwise."""
    for s in (left, right):
        if not asof_key_supported(s.dtype):
            raise ValueError(f"join_asof: on-key {s.name!r} has dtype "
                             f"{s.dtype}; numeric or temporal expected")
    if left.dtype == right.dtype:
        return left, right
    if left.dtype.is_floating() or right.dtype.is_floating():
        target = DataType.float64()
    else:
        for s in (left, right):
            if s.data.dtype == torch.uint64:
                raise ValueError("join_asof: a uint64 on-key needs a uint64 "
                                 "on-key on the other side")
        target = DataType.int64()
    return tuple(Series(s.name, target, data=s.data.to(target.to_torch()),
                        validity=s.validity) for s in (left, right))


def _usable(on: Series, by: List[Series]) -> Optional[torch.Tensor]:
    """Rows whose on-key and by keys are all valid; None when all are."""
    mask = None
    for s in [on] + list(by):
        if s.validity is not None:
            mask = s.validity if mask is None else mask & s.validity
    return mask


def _probe_host(lk: np.ndarray, lg: np.ndarray, rk: np.ndarray,
                rg: np.ndarray, right_rows: np.ndarray, seg: np.ndarray,
                strategy: int, allow_exact: bool,
                float_keys: bool) -> np.ndarray:
    """The rule of csrc/asof.hip in numpy.  lk, rk: uint64 encoded keys; rk,
    rg, right_rows are in sorted order."""
    nl = lk.shape[0]
    live = lg >= 0
    g = np.where(live, lg, 0)
    # one global search: rank-compress the keys, then (group, rank) packs
    # into an int64 that is sorted exactly as the right side is
    uniq = np.unique(np.concatenate([lk, rk]))
    width = np.int64(uniq.shape[0] + 1)
    packed_r = rg * width + np.searchsorted(uniq, rk).astype(np.int64)
    packed_l = g * width + np.searchsorted(uniq, lk).astype(np.int64)
    lower = np.searchsorted(packed_r, packed_l, side="left").astype(np.int64)
    upper = np.searchsorted(packed_r, packed_l, side="right").astype(np.int64)
    a, b = seg[g], seg[g + 1]
    if strategy == 0:
        pos = (upper if allow_exact else lower) - 1
        ok = pos >= a
    elif strategy == 1:
        pos = lower if allow_exact else upper
        ok = pos < b
    else:
        has_f, has_b = lower < b, lower - 1 >= a
        last = rk.shape[0] - 1
        kf = rk[np.clip(lower, 0, last)]
        kb = rk[np.clip(lower - 1, 0, last)]
        if float_keys:
            def decode(e):
                neg = (e >> np.uint64(63)) == 0
                return np.where(neg, ~e, e ^ np.uint64(1 << 63)) \
                    .view(np.float64)
            p = decode(lk)
            with np.errstate(invalid="ignore", over="ignore"):
                df = np.abs(decode(kf) - p)
                db = np.abs(decode(kb) - p)
            df = np.where(kf == lk, 0.0, df)
            nan_f, nan_b = np.isnan(df), np.isnan(db)
            fwd = np.where(nan_f | nan_b, nan_b, df <= db)
        else:
            fwd = (kf - lk) <= (lk - kb)      # uint64, wraps like the kernel
        pos = np.where(has_f & (fwd | ~has_b), lower, lower - 1)
        ok = has_f | has_b
    ok &= live
    out = np.full(nl, -1, dtype=np.int64)
    out[ok] = right_rows[pos[ok]]
    return out


def _group_ids(left_by: List[Series], right_by: List[Series], nl: int,
               nr: int, dev) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """(left gids, right gids, group count), consistent across the sides."""
    if not left_by:
        return (torch.zeros(nl, dtype=torch.int64, device=dev),
                torch.zeros(nr, dtype=torch.int64, device=dev), 1)
    # concat the by keys, group, then split
    merged = [Series.concat([l, r]) for l, r in zip(left_by, right_by)]
    gids, reps = rowops.groupby(merged)
    return gids[:nl], gids[nl:], len(reps)


def _sort_right(rk: torch.Tensor, rg: torch.Tensor,
                kept: Optional[torch.Tensor], num_groups: int):
    """Stable sort of the usable right rows by (group, key): (sorted keys,
    sorted gids, right_rows, seg_offsets)."""
    # rk ^ sign is a signed int64 that orders as the encoded key does
    sort_keys = [Series("__k", DataType.int64(), data=rk ^ _SIGN64)]
    if num_groups > 1:
        sort_keys.insert(0, Series("__g", DataType.int64(), data=rg))
    flags = [False] * len(sort_keys)
    rperm = rowops.argsort_multi(sort_keys, flags, flags)
    rk_s = rk[rperm].contiguous()
    rg_s = rg[rperm] if num_groups > 1 else rg
    right_rows = (rperm if kept is None else kept[rperm]).contiguous()
    seg = torch.zeros(num_groups + 1, dtype=torch.int64, device=rk.device)
    torch.cumsum(torch.bincount(rg_s, minlength=num_groups), 0, out=seg[1:])
    return rk_s, rg_s, right_rows, seg


def _probe(lk, lg, rk_s, rg_s, right_rows, seg, code: int, allow_exact: bool,
           float_keys: bool) -> torch.Tensor:
    if lk.is_cuda:
        return native_required().asof_probe(lk, lg, rk_s, right_rows, seg,
                                            code, allow_exact, float_keys)
    out = _probe_host(lk.numpy().view(np.uint64), lg.numpy(),
                      rk_s.numpy().view(np.uint64), rg_s.numpy(),
                      right_rows.numpy(), seg.numpy(), code, allow_exact,
                      float_keys)
    return torch.from_numpy(out)


def asof_match(left_keys: Series, right_keys: Series,
               left_by: List[Series], right_by: List[Series],
               strategy: str = "backward",
               allow_exact: bool = True) -> torch.Tensor:
    """Return right-row index per left row (-1 = no match)."""
    code = _check_strategy(strategy, allow_exact)
    left_keys, right_keys = _common_keys(left_keys, right_keys)
    nl, nr = len(left_keys), len(right_keys)
    dev = left_keys.device
    if nr == 0 or nl == 0:
        return torch.full((nl,), -1, dtype=torch.int64, device=dev)
    float_keys = left_keys.dtype.is_floating()
    lk = rowops._order_key_u64(left_keys).contiguous()
    rk = rowops._order_key_u64(right_keys)
    lg, rg, num_groups = _group_ids(left_by, right_by, nl, nr, dev)

    l_ok = _usable(left_keys, left_by)
    if l_ok is not None:
        lg = torch.where(l_ok, lg, torch.full_like(lg, -1))
    lg = lg.contiguous()
    r_ok = _usable(right_keys, right_by)
    kept = None
    if r_ok is not None:
        kept = torch.nonzero(r_ok).reshape(-1)
        if kept.numel() == 0:
            return torch.full((nl,), -1, dtype=torch.int64, device=dev)
        rk, rg = rk[kept], rg[kept]

    rk_s, rg_s, right_rows, seg = _sort_right(rk, rg, kept, num_groups)
    return _probe(lk, lg, rk_s, rg_s, right_rows, seg, code, allow_exact,
                  float_keys)


def run_asof_join(left: RecordBatch, right: RecordBatch,
                  left_on: str, right_on: str,
                  left_by: List[str], right_by: List[str],
                  strategy: str, right_cols: List[Tuple[str, str]]
                  ) -> RecordBatch:
    lk = left.column(left_on)
    rk = right.column(right_on)
    lb = [left.column(c) for c in left_by]
    rb = [right.column(c) for c in right_by]
    ridx = asof_match(lk, rk, lb, rb, strategy)
    cols = list(left.columns)
    for src, out in right_cols:
        cols.append(right.column(src).take(ridx).rename(out))
    return RecordBatch(cols, num_rows=len(left))
