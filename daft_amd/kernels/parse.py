"""Text <-> value conversion for casts, `to_date` and `to_datetime`.

A plain STRING column on the device is parsed by the kernels of
csrc/strparse.hip.  They answer a status per row: 0 parsed, 1 null, 2 "the
host must decide".  Only the status-2 rows travel to the host, run through the
same per-row Python the whole column ran through before (`_host_parse`, which
raises what it always raised), and are scattered back, so results are
unchanged by construction.  Integers and dates are formatted on the device
too; every other source type is stringified by `_host_to_string`.
"""
from __future__ import annotations

import datetime as _dt
from typing import Callable, Optional, Tuple

import torch

from ..schema import DataType, TypeKind
from ..series import Series

_INT_RANGE = {
    TypeKind.INT8: (-(1 << 7), (1 << 7) - 1),
    TypeKind.INT16: (-(1 << 15), (1 << 15) - 1),
    TypeKind.INT32: (-(1 << 31), (1 << 31) - 1),
    TypeKind.INT64: (-(1 << 63), (1 << 63) - 1),
    TypeKind.UINT8: (0, (1 << 8) - 1),
    TypeKind.UINT16: (0, (1 << 16) - 1),
    TypeKind.UINT32: (0, (1 << 32) - 1),
    TypeKind.UINT64: (0, (1 << 63) - 1),   # the upper half goes to the host
}
# same-width signed view of the unsigned storage types
_SIGNED_VIEW = {torch.uint16: torch.int16, torch.uint32: torch.int32,
                torch.uint64: torch.int64}
_DATETIME_SEP = {"%Y-%m-%d": 0, "%Y-%m-%d %H:%M:%S": ord(" "),
                 "%Y-%m-%dT%H:%M:%S": ord("T")}
_DAY_MIN = (_dt.date(1, 1, 1) - _dt.date(1970, 1, 1)).days
_DAY_MAX = (_dt.date(9999, 12, 31) - _dt.date(1970, 1, 1)).days


def _native():
    from . import native_required
    return native_required()


# ---------------------------------------------------------------------------
# host paths: one interpreter call per row
# ---------------------------------------------------------------------------

def _to_str(v) -> str:
    if isinstance(v, float):
        return repr(v)
    if isinstance(v, bytes):
        return v.decode("utf-8", "replace")
    return str(v)


def _host_to_string(s: Series) -> Series:
    vals = s.to_pylist()
    out = [None if v is None else _to_str(v) for v in vals]
    return Series.from_pylist(s.name, out, DataType.string(), device=s.device)


def _host_parse(s: Series, dtype: DataType,
                fmt: Optional[str] = None) -> Series:
    """STRING -> numeric or date by `int`, `float`, `Decimal` and
    `date.fromisoformat`; with `fmt`, -> date or timestamp by `strptime`."""
    vals = s.to_pylist()
    if fmt is not None:
        if dtype.kind == TypeKind.DATE:
            conv = lambda v: _dt.datetime.strptime(v, fmt).date()
        else:
            conv = lambda v: _dt.datetime.strptime(v, fmt)
        out = [None if v is None else conv(v) for v in vals]
    elif dtype.kind == TypeKind.DATE:
        out = [None if v is None else _dt.date.fromisoformat(v) for v in vals]
    else:
        if dtype.is_decimal():
            conv = lambda x: x  # Decimal(str) parse in from_pylist: exact
        elif dtype.is_floating():
            conv = float
        else:
            conv = int
        out = [None if v is None or v == "" else conv(v) for v in vals]
    return Series.from_pylist(s.name, out, dtype, device=s.device)


# ---------------------------------------------------------------------------
# parsing
# ---------------------------------------------------------------------------

_pow5_cache: dict = {}


def pow5_table(device) -> torch.Tensor:
    """int64 [651, 2]: for q in [-342, 308] the {low, high} 64-bit words of
    5^q as a 128-bit number with its top bit set, the binary exponent left
    out (Lemire, "Number parsing at a gigabyte per second", 2021).  For
    q >= 0 that is 5^q shifted up or truncated to 128 bits.  For q < 0 it is
    the reciprocal floor(2^b / 5^-q) + 1: to exactly 128 bits while 5^-q
    fits a 64-bit word (q >= -27), to twice the bits and then truncated to
    128 for the others."""
    key = str(device)
    if key not in _pow5_cache:
        rows = []
        for q in range(-342, 309):
            if q >= 0:
                c = 5 ** q
                shift = c.bit_length() - 128
                c = c >> shift if shift > 0 else c << -shift
            else:
                p = 5 ** -q
                z = p.bit_length()            # 2^(z - 1) < 5^-q < 2^z
                b = z + 127 if q >= -27 else 2 * z + 128
                c = (1 << b) // p + 1
                c >>= c.bit_length() - 128
            assert c.bit_length() == 128
            words = (c & ((1 << 64) - 1), c >> 64)
            rows.append([w - (1 << 64) if w >> 63 else w for w in words])
        _pow5_cache[key] = torch.tensor(rows, dtype=torch.int64,
                                        device=device)
    return _pow5_cache[key]


def device_target(s: Series, dtype: DataType) -> bool:
    """A plain device STRING column and a target the kernels parse."""
    if not (s.is_gpu() and s.dtype.kind == TypeKind.STRING and
            s.offsets is not None):
        return False
    k = dtype.kind
    if k == TypeKind.DECIMAL128:
        return dtype.precision <= 18
    return k in _INT_RANGE or k in (TypeKind.FLOAT32, TypeKind.FLOAT64,
                                    TypeKind.DATE)


def _run_kernel(s: Series, dtype: DataType,
                sep: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(values, status) of the kernel for `dtype`; values in the kernel's own
    type: int64, float64, or int32 days."""
    nat = _native()
    k = dtype.kind
    col = (s.offsets, s.data, s.validity)
    if k in _INT_RANGE:
        return nat.str_parse_int(*col, *_INT_RANGE[k])
    if k == TypeKind.DECIMAL128:
        return nat.str_parse_decimal(*col, dtype.scale,
                                     10 ** dtype.precision - 1)
    if k in (TypeKind.FLOAT32, TypeKind.FLOAT64):
        return nat.str_parse_float(*col, pow5_table(s.device))
    return nat.str_parse_datetime(*col, sep)


def _signed(t: torch.Tensor) -> torch.Tensor:
    return t.view(_SIGNED_VIEW[t.dtype]) if t.dtype in _SIGNED_VIEW else t


def _finish(s: Series, dtype: DataType, values: torch.Tensor,
            validity: Optional[torch.Tensor]) -> Series:
    """Kernel-typed values -> the storage type of `dtype`."""
    if dtype.kind not in (TypeKind.DECIMAL128, TypeKind.DATE,
                          TypeKind.TIMESTAMP):
        tdt = dtype.to_torch()
        if tdt in _SIGNED_VIEW:     # two's complement: truncate, then view
            values = values.to(_SIGNED_VIEW[tdt]).view(tdt)
        else:
            values = values.to(tdt)
    return Series(s.name, dtype, data=values, validity=validity)


def _merge(s: Series, dtype: DataType, values: torch.Tensor,
           status: torch.Tensor, host: Callable[[Series], Series]) -> Series:
    """Send the status-2 rows through `host`, scatter them back."""
    top = int(status.max().item()) if len(s) else 0   # the one sync
    if top == 0:
        return _finish(s, dtype, values, None)
    ok = status == 0
    if top == 2:
        rows = (status == 2).nonzero().reshape(-1)
        fixed = host(s.take(rows))
        values[rows] = _signed(fixed.data).to(values.dtype)
        ok[rows] = True if fixed.validity is None else fixed.validity
    return _finish(s, dtype, values, ok)


def parse_cast(s: Series, dtype: DataType) -> Series:
    """`cast` of a `device_target` column."""
    values, status = _run_kernel(s, dtype)
    return _merge(s, dtype, values, status, lambda t: _host_parse(t, dtype))


def _try_rows(t: Series, dtype: DataType) -> Series:
    """try_cast's salvage: each row alone, null where the host raises."""
    out = []
    for i in range(len(t)):
        try:
            out.append(_host_parse(t.slice(i, i + 1), dtype).to_pylist()[0])
        except Exception:
            out.append(None)
    return Series.from_pylist(t.name, out, dtype, device=t.device)


def try_parse_cast(s: Series, dtype: DataType) -> Series:
    """`try_cast` of a `device_target` column: only the status-2 rows are
    tried one by one."""
    values, status = _run_kernel(s, dtype)
    return _merge(s, dtype, values, status,
                  lambda t: _try_rows(t.cpu(), dtype).to(s.device))


def strptime_column(s: Series, fmt: str, dtype: DataType) -> Series:
    """`strptime(v, fmt)` per row as DATE or TIMESTAMP[us]; the ISO formats
    of a device column run on the kernel."""
    want_date = dtype.kind == TypeKind.DATE
    sep = _DATETIME_SEP.get(fmt)
    if s.is_dict() and s.is_gpu():
        s = s.dict_decode()
    if sep is None or (sep == 0) != want_date or \
            not device_target(s, DataType.date()):
        return _host_parse(s, dtype, fmt)
    values, status = _run_kernel(s, DataType.date(), sep)
    return _merge(s, dtype, values, status,
                  lambda t: _host_parse(t, dtype, fmt))


# ---------------------------------------------------------------------------
# formatting
# ---------------------------------------------------------------------------

def to_string(s: Series) -> Series:
    """`cast` to STRING: integers and dates of a device column are written by
    the format kernels, everything else by `str` on the host."""
    k = s.dtype.kind
    if s.is_gpu() and s.data is not None:
        nat = _native()
        out = None
        if k in _INT_RANGE and k != TypeKind.UINT64:
            v = _signed(s.data).to(torch.int64)
            if k in (TypeKind.UINT16, TypeKind.UINT32):
                v = v & _INT_RANGE[k][1]          # undo the sign extension
            out = nat.format_int(v, s.validity)
        elif k == TypeKind.DATE and s.data.dtype == torch.int32:
            d = s.data if s.validity is None else \
                torch.where(s.validity, s.data, torch.zeros_like(s.data))
            lo, hi = torch.stack(torch.aminmax(d)).tolist() \
                if len(s) else (0, 0)                         # one sync
            if _DAY_MIN <= lo and hi <= _DAY_MAX:
                out = nat.format_date(s.data, s.validity)
        if out is not None:
            return Series(s.name, DataType.string(), data=out[1],
                          offsets=out[0], validity=s.validity)
    return _host_to_string(s)
