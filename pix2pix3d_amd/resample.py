"""Frame resampling: Pillow's ``Image.resize`` on uint8 clips, bit for bit — the one thing the frame stack could not do where the frames are.

For 8-bit images PIL's resize is pure integer arithmetic on fixed-point coefficient tables, so "device bytes equal the CPU formulation" extends to "and
equal PIL's bytes".  The rules are csrc/video/p3d_video.h's ("frame resampling"); DESIGN.md section 2.1ab has the measurements.

    FILTERS                                                 ('nearest', 'box', 'bilinear', 'hamming', 'bicubic', 'lanczos')
    coefficients(in_size, out_size, filter, interval)       (bounds int32 [out, 2] = (xmin, count), weights int32 [out, ksize]): 22-bit fixed point, CPU
    nearest_indices(in_size, out_size)                      int32 [out]: the accumulated index table of PIL's NEAREST, CPU
    resize(frames, size, filter, box, out)                  uint8 [F, oh, ow(, bpp)]: horizontal pass into a uint8 intermediate, then the vertical pass
    thumbnails(frames, cell, filter)                        ``resize`` for ``views.image_grid``

Clips follow ``clips.check_frames``: uint8 [F, H, W, bpp] with bpp 2 .. 4, or [F, H, W] for one byte a pixel; contiguous pixels, any row and frame pitch.
The channels of a pixel are resampled independently.  That equals PIL for ``L``, ``RGB`` and ``RGBX``; it does NOT equal PIL's ``LA`` / ``RGBA`` path,
which premultiplies alpha before it resamples — premultiplication is out of scope.  ``nearest`` takes no ``box``.

CPU tensors run the integer torch formulation below, which is the definition; device tensors run the kernels of csrc/video/frame_resample.hip through
``clips.video_lib()`` (libp3d_video.so: the library of everything on uint8 clips) with the same bytes.  The tables are made on the host in Python
floats (IEEE double, one rounding per operator) and cached per (in, out, filter, interval, device): a repeated call uploads nothing and never
synchronises."""
import collections
import math
import operator

import torch

from . import _lib, clips

FILTERS = ('nearest', 'box', 'bilinear', 'hamming', 'bicubic', 'lanczos')
PRECISION_BITS = 22                                  # the fixed point of a weight: 32 - 8 - 2, PIL's
MAX_SIZE, TILE_W, TILE_H = (clips.HEADER.constants[k] for k in ('P3D_RESAMPLE_MAX_SIZE', 'P3D_RESAMPLE_TILE_W', 'P3D_RESAMPLE_TILE_H'))
CACHE_ENTRIES = 64                                   # tables kept; the least recently used one leaves first


# ---- the filters: f(x) and the support S --------------------------------------------------------------------------------------------------
def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_SEPARABLE = {'box': (_box, 0.5), 'bilinear': (_bilinear, 1.0), 'hamming': (_hamming, 1.0), 'bicubic': (_bicubic, 2.0), 'lanczos': (_lanczos, 3.0)}


def _check_filter(filter, who):
    if filter not in FILTERS:
        raise ValueError(f'{who}: filter must be one of {FILTERS}, got {filter!r}')


def _check_axis(in_size, out_size, who):
    for n, what in ((in_size, 'in_size'), (out_size, 'out_size')):
        if isinstance(n, bool) or int(n) != n or not 1 <= n <= MAX_SIZE:
            raise ValueError(f'{who}: {what} must be an integer in 1 .. {MAX_SIZE}, got {n!r}')
    return int(in_size), int(out_size)


def check_weights(weights):
    """The int32 bound of a table of 22-bit weights [out, ksize]: 255 * sum |k| + 2^21 < 2^31 for every output, so that no accumulator of a pass
    (int32, as PIL's are) can wrap; ValueError otherwise."""
    worst = int(weights.to(torch.int64).abs().sum(1).max()) if weights.numel() else 0
    if 255 * worst + (1 << (PRECISION_BITS - 1)) >= 1 << 31:
        raise ValueError(f'coefficients: 255 * {worst} + 2^21 reaches 2^31: the int32 accumulators of a pass would wrap')


def coefficients(in_size, out_size, filter, interval=None):
    """(bounds int32 [out_size, 2] = (xmin, count), weights int32 [out_size, ksize]) on the CPU for one axis of ``in_size`` pixels resampled to
    ``out_size`` from the source interval ``[in0, in1)`` (default the whole axis), rules 1 - 8 of the header: Python floats, in exactly that order."""
    _check_filter(filter, 'coefficients')
    if filter == 'nearest':
        raise ValueError("coefficients: 'nearest' has an index table (nearest_indices), not weights")
    in_size, out_size = _check_axis(in_size, out_size, 'coefficients')
    in0, in1 = (0.0, float(in_size)) if interval is None else (float(interval[0]), float(interval[1]))
    if not (0.0 <= in0 < in1 <= in_size):
        raise ValueError(f'coefficients: the interval [{in0}, {in1}) is empty or leaves the axis of {in_size} pixels')
    f, s = _SEPARABLE[filter]
    scale = (in1 - in0) / out_size
    fs = max(scale, 1.0)
    support = s * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    one = float(1 << PRECISION_BITS)
    bounds, weights = [], []
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), in_size) - xmin
        w = [f((i + xmin - center + 0.5) * ss) for i in range(count)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        bounds.append((xmin, count))
        weights.append(k + [0] * (ksize - count))
    bounds, weights = torch.tensor(bounds, dtype=torch.int32).reshape(out_size, 2), torch.tensor(weights, dtype=torch.int32).reshape(out_size, ksize)
    check_weights(weights)
    return bounds, weights


def nearest_indices(in_size, out_size):
    """int32 [out_size] on the CPU: the source index of every output of PIL's NEAREST, by ACCUMULATION (s = in / out; xo = s * 0.5; idx = min(int(xo),
    in - 1), xo += s) — the closed form int((x + 0.5) * in / out) differs from it at some sizes (512 -> 300)."""
    in_size, out_size = _check_axis(in_size, out_size, 'nearest_indices')
    s = in_size / out_size
    xo = s * 0.5
    idx = []
    for _ in range(out_size):
        idx.append(min(int(xo), in_size - 1))
        xo += s
    return torch.tensor(idx, dtype=torch.int32)


# ---- the table cache ------------------------------------------------------------------------------------------------------------------------
_cache = collections.OrderedDict()                   # (in, out, filter, interval, device) -> tuple of tensors on that device
_cache_stats = {'hits': 0, 'builds': 0}


def cache_info():
    """{'hits', 'builds', 'entries'}: ``builds`` counts the tables made (and, for a device, uploaded); a repeated call only adds to ``hits``."""
    return dict(_cache_stats, entries=len(_cache))


def cache_clear():
    _cache.clear()
    _cache_stats.update(hits=0, builds=0)


def _tables(in_size, out_size, filter, interval, device, shifted=False):
    """The tables of one axis on ``device``, made once: (indices,) for 'nearest', else (bounds, weights, first, last) with [first, last) the source
    span the axis reads — bounds[0].xmin up to the end of the last output's bounds.  ``shifted``: xmin counted from ``first``."""
    key = (in_size, out_size, filter, interval, str(device), shifted)
    found = _cache.get(key)
    if found is not None:
        _cache.move_to_end(key)
        _cache_stats['hits'] += 1
        return found
    if filter == 'nearest':
        made = (nearest_indices(in_size, out_size).to(device),)
    else:
        bounds, weights = coefficients(in_size, out_size, filter, interval)
        first, last = int(bounds[0, 0]), int(bounds[-1, 0] + bounds[-1, 1])
        if shifted:
            bounds[:, 0] -= first
        made = (bounds.to(device), weights.to(device), first, last)
    _cache[key] = made
    _cache_stats['builds'] += 1
    while len(_cache) > CACHE_ENTRIES:
        _cache.popitem(last=False)
    return made


# ---- the passes: the definition, on the tensor's device -------------------------------------------------------------------------------------
def pass_sums(src, axis, bounds, weights):
    """The UNCLAMPED sums of one pass, int32: 2^21 + sum_i k[i] * src[xmin + i] along ``axis`` of src (uint8, any shape), before the shift and the
    clip.  One gather and one multiply-add per tap."""
    out_size, ksize = weights.shape
    xmin, count = bounds[:, 0].long(), bounds[:, 1].long()
    n = src.shape[axis]
    shape = [1] * src.ndim
    shape[axis] = out_size
    acc = torch.full(list(src.shape[:axis]) + [out_size] + list(src.shape[axis + 1:]), 1 << (PRECISION_BITS - 1), dtype=torch.int32, device=src.device)
    for i in range(ksize):
        live = count > i
        if not bool(live.any()):
            break
        k = torch.where(live, weights[:, i], torch.zeros_like(weights[:, i]))
        acc += src.index_select(axis, (xmin + i).clamp(max=n - 1)).to(torch.int32) * k.reshape(shape)
    return acc


def _pass_torch(src, axis, bounds, weights):
    return (pass_sums(src, axis, bounds, weights) >> PRECISION_BITS).clamp(0, 255).to(torch.uint8)


def _pass_device(src, axis, bounds, weights, dst):
    entry = clips.video_lib().p3d_frame_resample_rows if axis == 2 else clips.video_lib().p3d_frame_resample_columns
    code = entry(*clips.clip_args(src), clips.bpp_of(src), *clips.clip_args(dst)[:3], dst.shape[axis], _lib.ptr(bounds), _lib.ptr(weights), weights.shape[1],
                 _lib.stream_of(dst))
    clips.check(code, 'frame_resample_rows' if axis == 2 else 'frame_resample_columns')


def _nearest(src, xidx, yidx, dst):
    if not src.is_cuda:
        dst.copy_(src.index_select(1, yidx.long()).index_select(2, xidx.long()))
        return
    clips.check(clips.video_lib().p3d_frame_resample_nearest(*clips.clip_args(src), clips.bpp_of(src), *clips.clip_args(dst)[:3], dst.shape[1], dst.shape[2],
                                                             _lib.ptr(xidx), _lib.ptr(yidx), _lib.stream_of(dst)), 'frame_resample_nearest')


# ---- resize ------------------------------------------------------------------------------------------------------------------------------
def _check_size(size, who):
    pair = tuple(size) if isinstance(size, (tuple, list)) else (size, size)
    try:
        pair = tuple(operator.index(n) for n in pair if not isinstance(n, bool))
    except TypeError:
        pair = ()
    if len(pair) != 2:
        raise ValueError(f'{who}: size must be (width, height) or an int, got {size!r}')
    if not all(1 <= n <= MAX_SIZE for n in pair):
        raise ValueError(f'{who}: size must be within 1 .. {MAX_SIZE} a side, got {size!r}')
    return pair


def _check_box(box, h, w, filter, who):
    """((x0, x1) or None, (y0, y1) or None): the interval of each axis, None for the whole axis."""
    if box is None:
        return None, None
    if filter == 'nearest':
        raise ValueError(f"{who}: 'nearest' takes no box")
    try:
        x0, y0, x1, y1 = (float(v) for v in box)
    except (TypeError, ValueError):
        raise ValueError(f'{who}: box must be (x0, y0, x1, y1), got {box!r}')
    if not all(math.isfinite(v) for v in (x0, y0, x1, y1)) or not (x0 < x1 and y0 < y1):
        raise ValueError(f'{who}: the box {box!r} is empty or inverted')
    if x0 < 0 or y0 < 0 or x1 > w or y1 > h:
        raise ValueError(f'{who}: the box {box!r} leaves the {w} x {h} image')
    return (None if (x0, x1) == (0.0, float(w)) else (x0, x1)), (None if (y0, y1) == (0.0, float(h)) else (y0, y1))


def resize(frames, size, filter='lanczos', box=None, out=None):
    """``PIL.Image.resize(size, filter, box)`` of every frame of a uint8 clip [F, H, W, bpp] (bpp 2 .. 4) or [F, H, W], where the clip is: uint8
    [F, oh, ow(, bpp)].  ``size``: (width, height) or an int for both; ``filter``: one of ``FILTERS``; ``box``: (x0, y0, x1, y1) floats, the source
    region, PIL's (not with 'nearest'); ``out``: a clip to write into, any row and frame pitch, apart from ``frames``.

    The horizontal pass runs first, into a uint8 intermediate of the source rows the vertical pass reads, then the vertical pass; an axis whose size
    is unchanged and whose interval is the whole axis is skipped, and with both skipped the result is a copy.  Launches: 0 for F == 0 and for a
    copy, 1 for 'nearest' and for a single axis, 2 for both axes.  The channels of a pixel are resampled independently: PIL's ``L``, ``RGB`` and
    ``RGBX`` — not its ``LA`` / ``RGBA`` path, which premultiplies alpha (out of scope).  Every argument error is a ValueError before any launch."""
    _check_filter(filter, 'resize')
    f, h, w = clips.check_frames(frames, 'resize: frames', bpp=(1, 2, 3, 4))
    ow, oh = _check_size(size, 'resize')
    if f and not (1 <= h <= MAX_SIZE and 1 <= w <= MAX_SIZE):
        raise ValueError(f'resize: frames of {w} x {h} pixels: every side is 1 .. {MAX_SIZE}')
    box_x, box_y = _check_box(box, h, w, filter, 'resize')
    out = clips.check_out(out, [f, oh, ow] + list(frames.shape[3:]), frames, 'resize')
    if f == 0:
        return out
    dev = frames.device
    if filter == 'nearest':
        (xidx,), (yidx,) = _tables(w, ow, 'nearest', None, dev), _tables(h, oh, 'nearest', None, dev)
        _nearest(frames, xidx, yidx, out)
        return out
    need_x, need_y = ow != w or box_x is not None, oh != h or box_y is not None
    if not need_x and not need_y:
        out.copy_(frames)
        return out
    run = _pass_device if frames.is_cuda else (lambda src, axis, b, k, dst: dst.copy_(_pass_torch(src, axis, b, k)))
    src = frames
    if need_y:
        bounds_y, weights_y, first, last = _tables(h, oh, filter, box_y, dev, shifted=need_x)
    if need_x:
        if need_y:
            src = src[:, first:last]                                           # only the rows the vertical pass reads: a slice, any row pitch will do
        dst = out if not need_y else torch.empty([f, src.shape[1], ow] + list(frames.shape[3:]), dtype=torch.uint8, device=dev)
        run(src, 2, *_tables(w, ow, filter, box_x, dev)[:2], dst)
        src = dst
    if need_y:
        run(src, 1, bounds_y, weights_y, out)
    return out


def thumbnails(frames, cell, filter='lanczos'):
    """``resize(frames, cell, filter)`` for ``views.image_grid``: every frame of [N, H, W(, C)] at ``cell`` = (width, height) or an int."""
    return resize(frames, cell, filter)
