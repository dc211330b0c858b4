"""Image kernels (ref: /root/reference/src/daft-image/src/series.rs —
decode :73, encode :99, resize :123, crop :157, to_mode :186, to_tensor
:257).  Decode/encode run on host (PIL); resize is a HIP bilinear kernel
over variable-size device-resident images."""
from __future__ import annotations

import io
import os
from typing import Optional

import numpy as np
import torch

from ..expressions.expressions import Expression, ScalarFn, _Namespace
from ..schema import DataType, TypeKind
from ..series import Series
from ..kernels import _is_gpu, native_required

_MODE_CHANNELS = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4}
_MODE_CODE = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4}


def _image_struct(name, datas, heights, widths, channels, mode_codes,
                  validity, device) -> Series:
    """Build an Image(mode=None) struct series from per-row raw buffers."""
    offs = np.zeros(len(datas) + 1, dtype=np.int64)
    for i, d in enumerate(datas):
        offs[i + 1] = offs[i] + len(d)
    blob = b"".join(datas)
    data_child = Series(
        "data", DataType.binary(),
        data=torch.frombuffer(bytearray(blob), dtype=torch.uint8)
        if blob else torch.zeros(0, dtype=torch.uint8),
        offsets=torch.from_numpy(offs))
    ch = Series("channel", DataType.uint16(),
                data=torch.tensor(channels, dtype=torch.int16)
                .view(torch.uint16))
    h = Series("height", DataType.uint32(),
               data=torch.tensor(heights, dtype=torch.int32)
               .view(torch.uint32))
    w = Series("width", DataType.uint32(),
               data=torch.tensor(widths, dtype=torch.int32)
               .view(torch.uint32))
    m = Series("mode", DataType.uint8(),
               data=torch.tensor(mode_codes, dtype=torch.uint8))
    s = Series(name, DataType.image(), children=[data_child, ch, h, w, m],
               validity=validity, length=len(datas))
    return s.to(device) if str(device) != "cpu" else s


def _decode_chunk(args):
    """Process-pool worker: inputs AND outputs travel via shared memory —
    only (segment name, offsets, dims) cross the pipe, so neither side
    ever pickles pixel payloads."""
    in_name, in_offs, valid_mask, mode, on_error = args
    import io as _io
    from multiprocessing import shared_memory as _shm

    import numpy as _np
    from PIL import Image as _PIL
    src = _shm.SharedMemory(name=in_name)
    buf = _np.frombuffer(src.buf, dtype=_np.uint8)
    parts = []
    dims = []
    total = 0
    k = len(in_offs) - 1
    for i in range(k):
        if valid_mask is not None and not valid_mask[i]:
            dims.append((0, 0, 0, False))
            continue
        v = bytes(buf[in_offs[i]:in_offs[i + 1]])
        if len(v) == 0:
            dims.append((0, 0, 0, False))
            continue
        try:
            img = _PIL.open(_io.BytesIO(v)).convert(mode)
            arr = _np.asarray(img, dtype=_np.uint8)
            if arr.ndim == 2:
                arr = arr[:, :, None]
            parts.append(arr)
            dims.append(arr.shape + (True,))
            total += arr.nbytes
        except Exception:
            if on_error == "raise":
                raise
            dims.append((0, 0, 0, False))
    del buf            # release the exported view before closing the mmap
    src.close()
    seg = _shm.SharedMemory(create=True, size=max(total, 1))
    off = 0
    for arr in parts:
        nb = arr.nbytes
        _np.frombuffer(seg.buf, dtype=_np.uint8,
                       count=nb, offset=off)[:] = arr.reshape(-1)
        off += nb
    seg_name = seg.name
    seg.close()
    # the parent owns the unlink; stop this worker's resource tracker
    # from double-reporting the segment at shutdown
    try:
        from multiprocessing import resource_tracker as _rt
        _rt.unregister("/" + seg_name, "shared_memory")
    except Exception:
        pass
    return seg_name, total, dims


_DECODE_POOL = None


def _decode_pool_struct(series, mode, on_error, device):
    """Chunked process-pool decode straight into the Image struct: the
    input binary column's contiguous buffer is published ONCE as a
    shared-memory segment; workers decode their row ranges from it and
    return their pixels in shared memory — no per-image Python objects
    and no payload pickling in either direction."""
    global _DECODE_POOL
    import concurrent.futures as fut
    import multiprocessing as mp
    from multiprocessing import shared_memory as _shmmod
    name = series.name
    cpu = series.cpu()
    data_np = cpu.data.contiguous().numpy() if cpu.data is not None         else np.zeros(0, dtype=np.uint8)
    offs_np = cpu.offsets.numpy()
    valid_np = cpu.validity.numpy() if cpu.validity is not None else None
    n = len(series)
    workers = min(96, max(8, (os.cpu_count() or 8) // 2))
    if _DECODE_POOL is None:
        _DECODE_POOL = fut.ProcessPoolExecutor(
            max_workers=workers, mp_context=mp.get_context("fork"))
    shm_in = _shmmod.SharedMemory(create=True,
                                  size=max(int(data_np.nbytes), 1))
    np.frombuffer(shm_in.buf, dtype=np.uint8,
                  count=data_np.nbytes)[:] = data_np
    chunk = max(64, n // (workers * 4))
    jobs = []
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        jobs.append((shm_in.name, offs_np[lo:hi + 1].copy(),
                     valid_np[lo:hi].copy() if valid_np is not None
                     else None, mode, on_error))
    try:
        outs = list(_DECODE_POOL.map(_decode_chunk, jobs))
    finally:
        shm_in.close()
        shm_in.unlink()
    vals = [None] * n   # only used for length below
    total = sum(t for _n, t, _d in outs)
    blob_t = torch.empty(max(total, 0), dtype=torch.uint8)
    blob_np = blob_t.numpy()
    off = 0
    for seg_name, t, _d in outs:
        seg = _shmmod.SharedMemory(name=seg_name)
        if t:
            blob_np[off:off + t] = np.frombuffer(seg.buf, dtype=np.uint8,
                                                 count=t)
        off += t
        seg.close()
        seg.unlink()
    dims = np.array([d for _n, _t, ds in outs for d in ds], dtype=np.int64)
    if dims.size == 0:
        dims = dims.reshape(0, 4)
    hs, ws, cs, ok = dims[:, 0], dims[:, 1], dims[:, 2], dims[:, 3]
    nbytes = hs * ws * cs
    offs = np.zeros(len(vals) + 1, dtype=np.int64)
    np.cumsum(nbytes, out=offs[1:])
    data_child = Series(
        "data", DataType.binary(),
        data=blob_t,
        offsets=torch.from_numpy(offs))
    ch = Series("channel", DataType.uint16(),
                data=torch.from_numpy(cs.astype(np.int16)).view(torch.uint16))
    h = Series("height", DataType.uint32(),
               data=torch.from_numpy(hs.astype(np.int32)).view(torch.uint32))
    w = Series("width", DataType.uint32(),
               data=torch.from_numpy(ws.astype(np.int32)).view(torch.uint32))
    mcode = _MODE_CODE.get(mode, 3)
    m = Series("mode", DataType.uint8(),
               data=torch.from_numpy(
                   np.where(ok.astype(bool), mcode, 0).astype(np.uint8)))
    validity = None
    if not bool(ok.all()):
        validity = torch.from_numpy(ok.astype(bool))
    s = Series(name, DataType.image(),
               children=[data_child, ch, h, w, m],
               validity=validity, length=len(vals))
    return s.to(device) if str(device) != "cpu" else s


def decode_series(s: Series, mode: str = "RGB",
                  on_error: str = "raise") -> Series:
    """binary (encoded JPEG/PNG/...) -> Image struct.

    Host decode on a thread pool (Pillow releases the GIL in its codecs);
    decoded pixels land in HBM for the HIP resize/tensor kernels."""
    import concurrent.futures as fut
    from PIL import Image as PILImage

    if s.is_dict():
        # repeated blobs (dict-encoded binary): decode each DISTINCT image
        # once, then gather the struct by code
        vocab = decode_series(s.children[0].rename(s.name), mode, on_error)
        out = vocab.take(s.data.to(torch.int64), has_neg=False)
        if s.validity is not None:
            v = out.validity & s.validity if out.validity is not None \
                else s.validity
            out = Series(out.name, out.dtype, data=out.data,
                         validity=v, offsets=out.offsets,
                         children=out.children, length=len(out))
        return out

    ncpu = os.cpu_count() or 8
    if len(s) >= 4096 and ncpu >= 16 and s.pyobjs is None and \
            s.offsets is not None:
        # decode-pool path: chunked PROCESS pool with shared-memory
        # transport in both directions — the "decode pool saturating the
        # link" design on many-core hosts
        return _decode_pool_struct(s, mode, on_error, s.device)
    vals = s.cpu().to_pylist()

    def one(v):
        if v is None:
            return None
        try:
            img = PILImage.open(io.BytesIO(v)).convert(mode)
            arr = np.asarray(img, dtype=np.uint8)
            if arr.ndim == 2:
                arr = arr[:, :, None]
            return arr
        except Exception:
            if on_error == "raise":
                raise
            return None

    if len(vals) >= 64:
        # Pillow's codecs release the GIL; 3x oversubscription hides the
        # GIL-held numpy-conversion phase (measured +17% vs 1x on 8 cores)
        workers = min(64, 3 * ncpu)
        with fut.ThreadPoolExecutor(max_workers=workers) as ex:
            arrs = list(ex.map(one, vals))
    else:
        arrs = [one(v) for v in vals]

    datas, hs, ws, cs, ms, valid = [], [], [], [], [], []
    for arr in arrs:
        if arr is None:
            datas.append(b"")
            hs.append(0)
            ws.append(0)
            cs.append(0)
            ms.append(0)
            valid.append(False)
        else:
            datas.append(arr.tobytes())
            hs.append(arr.shape[0])
            ws.append(arr.shape[1])
            cs.append(arr.shape[2])
            ms.append(_MODE_CODE.get(mode, 3))
            valid.append(True)
    validity = torch.tensor(valid, dtype=torch.bool) \
        if not all(valid) else None
    return _image_struct(s.name, datas, hs, ws, cs, ms, validity, s.device)


def encode_series(s: Series, fmt: str = "PNG") -> Series:
    """Image struct -> encoded binary (host)."""
    from PIL import Image as PILImage
    cpu = s.cpu()
    data, ch, h, w, _m = cpu.children
    offs = data.offsets.numpy()
    blob = data.data.numpy()
    out = []
    for i in range(len(cpu)):
        if cpu.validity is not None and not bool(cpu.validity[i]):
            out.append(None)
            continue
        hh = int(h.data.view(torch.int32)[i])
        ww = int(w.data.view(torch.int32)[i])
        cc = int(ch.data.view(torch.int16)[i])
        arr = blob[offs[i]:offs[i + 1]].reshape(hh, ww, cc)
        mode = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[cc]
        buf = io.BytesIO()
        PILImage.fromarray(arr.squeeze() if cc == 1 else arr, mode).save(
            buf, format=fmt)
        out.append(buf.getvalue())
    res = Series.from_pylist(s.name, out, DataType.binary())
    return res.to(s.device) if s.is_gpu() else res


def resize_series(s: Series, h: int, w: int) -> Series:
    """Image struct -> FixedShapeImage (HIP bilinear kernel on GPU).

    Bilinear with half-pixel centres: output pixel o samples the source at
    ((2*o+1)*in - out) / (2*out), neighbours clamped to the image, and the
    result rounds half up.  Both devices follow this rule.  The source
    rows must be 3-channel; a null row, or one without pixels, gives zeros
    and keeps its null."""
    assert s.dtype.kind == TypeKind.IMAGE, f"resize expects Image, got {s.dtype!r}"
    if int(h) < 1 or int(w) < 1:
        raise ValueError(f"image.resize: output size must be >= 1x1, got "
                         f"{h}x{w}")
    data, ch, hh, ww, _m = s.children
    channels = 3  # fixed-shape output mode RGB (round-1)
    n = len(s)
    out_dt = DataType.fixed_shape_image("RGB", h, w)
    src_h = hh.data.view(torch.int32)
    src_w = ww.data.view(torch.int32)
    if s.validity is not None:
        # whatever lies under a null row is not an image: resize it as 0x0
        zero = torch.zeros_like(src_h)
        src_h = torch.where(s.validity, src_h, zero)
        src_w = torch.where(s.validity, src_w, zero)
    # the kernel strides the pixels by `channels`: an L or RGBA row would be
    # read with the wrong stride (and, for L, past its bytes)
    bad = (ch.data.view(torch.int16) != channels) & (src_h > 0) & (src_w > 0)
    if n and bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise ValueError(
            f"image.resize: row {i} has {int(ch.data.view(torch.int16)[i])} "
            f"channel(s); resize takes {channels}-channel (RGB) images only "
            f"- decode with mode='RGB' first")
    if _is_gpu(s):
        flat = native_required().image_resize(
            data.data, data.offsets[:-1].contiguous(), src_h.contiguous(),
            src_w.contiguous(), channels, h, w)
        child = Series("item", DataType.uint8(), data=flat)
        return Series(s.name, out_dt, children=[child],
                      validity=s.validity, length=n)
    # CPU fallback: torch bilinear per row
    offs = data.offsets
    out = torch.zeros(n * h * w * channels, dtype=torch.uint8)
    blob = data.data
    for i in range(n):
        ih, iw = int(src_h[i]), int(src_w[i])
        if ih <= 0 or iw <= 0:
            continue
        arr = blob[offs[i]:offs[i + 1]].reshape(ih, iw, channels)
        t = arr.permute(2, 0, 1).unsqueeze(0).to(torch.float32)
        r = torch.nn.functional.interpolate(
            t, size=(h, w), mode="bilinear", align_corners=False)
        # round half up, as the kernel does (torch.round is half-to-even)
        r8 = (r + 0.5).floor().clamp(0, 255).to(torch.uint8).squeeze(0) \
            .permute(1, 2, 0).contiguous()
        out[i * h * w * channels:(i + 1) * h * w * channels] = r8.reshape(-1)
    child = Series("item", DataType.uint8(), data=out)
    return Series(s.name, out_dt, children=[child], validity=s.validity,
                  length=n)


def to_tensor_series(s: Series, dtype=None) -> Series:
    """FixedShapeImage -> FixedShapeTensor float32 in [0,1], CHW."""
    assert s.dtype.kind == TypeKind.FIXED_SHAPE_IMAGE
    hgt, wdt = s.dtype.shape
    c = _MODE_CHANNELS.get(s.dtype.image_mode or "RGB", 3)
    n = len(s)
    hwc = s.children[0].data.reshape(n, hgt, wdt, c)
    chw = hwc.permute(0, 3, 1, 2).to(torch.float32) / 255.0
    child = Series("item", DataType.float32(),
                   data=chw.reshape(-1).contiguous())
    return Series(s.name, DataType.fixed_shape_tensor(
        DataType.float32(), (c, hgt, wdt)), children=[child],
        validity=s.validity, length=n)


def crop_series(s: Series, x: int, y: int, w: int, h: int) -> Series:
    """FixedShapeImage crop (device slice)."""
    assert s.dtype.kind == TypeKind.FIXED_SHAPE_IMAGE
    H, W = s.dtype.shape
    c = _MODE_CHANNELS.get(s.dtype.image_mode or "RGB", 3)
    n = len(s)
    img = s.children[0].data.reshape(n, H, W, c)
    out = img[:, y:y + h, x:x + w, :].contiguous()
    child = Series("item", DataType.uint8(), data=out.reshape(-1))
    return Series(s.name, DataType.fixed_shape_image(
        s.dtype.image_mode or "RGB", h, w), children=[child],
        validity=s.validity, length=n)




_LUMA = (0.299, 0.587, 0.114)  # ITU-R 601-2, matching PIL convert("L")


def to_mode_series(s: Series, mode: str) -> Series:
    """Convert FixedShapeImage between L/RGB/RGBA on the device (ref:
    /root/reference/src/daft-image/src/series.rs:186 to_mode)."""
    assert s.dtype.kind == TypeKind.FIXED_SHAPE_IMAGE, \
        f"to_mode expects FixedShapeImage, got {s.dtype!r}"
    src_mode = s.dtype.image_mode or "RGB"
    if mode == src_mode:
        return s
    h, w = s.dtype.shape
    cs = _MODE_CHANNELS[src_mode]
    cd = _MODE_CHANNELS[mode]
    n = len(s)
    img = s.children[0].data.reshape(n, h, w, cs)
    f = img.to(torch.float32)
    if src_mode in ("L", "LA"):
        lum = f[..., 0]
        alpha = f[..., 1] if src_mode == "LA" else None
    else:
        lum = (f[..., 0] * _LUMA[0] + f[..., 1] * _LUMA[1]
               + f[..., 2] * _LUMA[2])
        alpha = f[..., 3] if src_mode == "RGBA" else None
    if alpha is None:
        alpha = torch.full_like(lum, 255.0)
    if mode == "L":
        out = lum.unsqueeze(-1)
    elif mode == "LA":
        out = torch.stack([lum, alpha], dim=-1)
    elif mode in ("RGB", "RGBA"):
        if src_mode in ("L", "LA"):
            rgb = lum.unsqueeze(-1).expand(n, h, w, 3)
        else:
            rgb = f[..., :3]
        out = torch.cat([rgb, alpha.unsqueeze(-1)], dim=-1) \
            if mode == "RGBA" else rgb
    else:
        raise ValueError(f"unknown image mode {mode!r}")
    data = out.round().clamp(0, 255).to(torch.uint8).reshape(-1)
    child = Series("item", DataType.uint8(), data=data.contiguous())
    return Series(s.name, DataType.fixed_shape_image(mode, h, w),
                  children=[child], validity=s.validity, length=n)


class ImageNamespace(_Namespace):
    def decode(self, mode: str = "RGB", on_error: str = "raise"):
        return self._fn("image_decode", decode_series, DataType.image(),
                        mode, on_error)

    def encode(self, image_format: str = "PNG"):
        return self._fn("image_encode", encode_series, DataType.binary(),
                        image_format)

    def resize(self, h: int, w: int):
        return self._fn("image_resize", resize_series,
                        DataType.fixed_shape_image("RGB", h, w), h, w)

    def to_tensor(self):
        def ret(fields):
            dt = fields[0].dtype
            c = _MODE_CHANNELS.get(dt.image_mode or "RGB", 3)
            return DataType.fixed_shape_tensor(DataType.float32(),
                                               (c,) + tuple(dt.shape))
        return self._fn("image_to_tensor", to_tensor_series, ret)

    def to_mode(self, mode: str):
        def ret(fields):
            dt = fields[0].dtype
            return DataType.fixed_shape_image(mode, *dt.shape)
        return self._fn("image_to_mode", to_mode_series, ret, mode)

    def crop(self, x: int, y: int, w: int, h: int):
        def ret(fields):
            dt = fields[0].dtype
            return DataType.fixed_shape_image(dt.image_mode or "RGB", h, w)
        return self._fn("image_crop", crop_series, ret, x, y, w, h)


def _image_attr(name, child_idx, view_dt, out_dt):
    def make(expr):
        from ..expressions.expressions import Expression, ScalarFn, _to_node

        def run(s: Series) -> Series:
            assert s.dtype.kind == TypeKind.IMAGE, \
                f"{name} expects Image, got {s.dtype!r}"
            c = s.children[child_idx]
            data = c.data.view(view_dt).to(torch.int64) if view_dt else \
                c.data.to(torch.int64)
            return Series(s.name, out_dt, data=data.to(torch.int32),
                          validity=s.validity)
        return Expression(ScalarFn(name, run, [_to_node(expr)], out_dt))
    make.__name__ = name
    return make


image_height = _image_attr("image_height", 2, torch.int32,
                           DataType.int32())
image_width = _image_attr("image_width", 3, torch.int32, DataType.int32())
image_channel = _image_attr("image_channel", 1, torch.int16,
                            DataType.int32())


def image_mode(expr):
    from ..expressions.expressions import Expression, ScalarFn, _to_node

    def run(s: Series) -> Series:
        codes = s.children[4].data.to(torch.int64).cpu().tolist()
        names = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA", 0: None}
        out = [names.get(c) for c in codes]
        r = Series.from_pylist(s.name, out, DataType.string())
        return r.to(s.device) if s.is_gpu() else r
    return Expression(ScalarFn("image_mode", run, [_to_node(expr)],
                               DataType.string()))


def image_attribute(expr, attr: str):
    return {"height": image_height, "width": image_width,
            "channel": image_channel, "mode": image_mode}[attr](expr)


def image_hash(expr, algorithm: str = "average", hash_size: int = 8):
    """Perceptual image hash (average-hash): resize to hash_size^2 luma,
    threshold at the mean -> bit string (capability of daft's
    image hash fns)."""
    from ..expressions.expressions import Expression, ScalarFn, _to_node

    def run(s: Series) -> Series:
        small = resize_series(s, hash_size, hash_size)
        lum = to_mode_series(small, "L")
        n = len(s)
        px = lum.children[0].data.reshape(n, hash_size * hash_size) \
            .to(torch.float32)
        mean = px.mean(dim=1, keepdim=True)
        bits = (px > mean).cpu().numpy()
        out = ["".join("1" if b else "0" for b in row) for row in bits]
        r = Series.from_pylist(s.name, out, DataType.string())
        return r.to(s.device) if s.is_gpu() else r
    return Expression(ScalarFn("image_hash", run, [_to_node(expr)],
                               DataType.string()))


def convert_image(expr, mode: str):
    from ..expressions.expressions import Expression as E, _to_node
    e = expr if isinstance(expr, E) else E(_to_node(expr))
    return e.image.to_mode(mode)


def decode_image(expr, mode: str = "RGB", on_error: str = "raise"):
    from ..expressions.expressions import Expression as E, _to_node
    e = expr if isinstance(expr, E) else E(_to_node(expr))
    return e.image.decode(mode, on_error)


def encode_image(expr, image_format: str = "PNG"):
    from ..expressions.expressions import Expression as E, _to_node
    e = expr if isinstance(expr, E) else E(_to_node(expr))
    return e.image.encode(image_format)


def image_to_tensor(expr):
    from ..expressions.expressions import Expression as E, _to_node
    e = expr if isinstance(expr, E) else E(_to_node(expr))
    return e.image.to_tensor()
