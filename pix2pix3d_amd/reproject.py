"""Cross-view consistency: how well two views of one latent agree in 3D — the claim a 3D-aware generator exists to make, and the one quality measure that
needs no feature network.  The pixels of one view are lifted to world points along their rays, projected into another camera, the nearest point per target
pixel is kept, labels and colours are carried across and compared with what the generator actually rendered there.  The same forward warp is a cheap
novel-view preview of a rendered frame (``warp``).  The reference has no code for any of this.

Three primitives with fixed rules (csrc/regions/p3d_regions.h states them; the kernels live in libp3d_regions.so beside
the region tools and the agreement metrics and are called through ``regions.regions_lib()``), each with a torch formulation that CPU tensors take — the definition: fp64 element-wise ops in the
header's order — and ONE device launch whose bytes equal it:

    splat(points, cameras, size, radius, valid)        int64 [F, H, W]: per target pixel the smallest key zkey * 2^32 + index of the points landing there
    resolve(zbuf, source, fill, target_points, ...)    (warped uint8 [F, H, W(, C)], status uint8 [F, H, W][, index int32 [F, H, W]]); counts int64 [5]
    difference_histogram(a, b, where, match)           int64 [256]: |a - b| per channel of the pixels with ``where == match``

``points(depth, cameras)`` makes the kernels' inputs from the project's own ``RaySampler`` (plain torch ops: no byte claim is made for them).  Every counter
ACCUMULATES into the caller's zeroed int64 tensor without a host synchronisation; ``metrics_from_consistency`` does the one host read and the fp64 divisions.
``consistency_counts`` composes the primitives with ``evaluate.confusion`` (5 launches of libp3d_regions.so per call with labels, 3 without, however many
pairs), ``Consistency`` accumulates, ``video_consistency`` measures the frames of a camera path against each other and ``EditSession.consistency`` /
``SketchSession.consistency`` the current frame against a second camera on the kept planes."""
import ctypes
import math

import numpy as np
import torch

from . import _lib, evaluate, regions
from .edit import MAX_SIZE

_C = regions.HEADER.constants                               # p3d_regions.h states every bound and code of the view functions
EMPTY = _C['P3D_VIEW_EMPTY']                                # a z-buffer cell nothing landed on
# the status of a target pixel
HOLE, CONSISTENT, BEHIND, IN_FRONT, NO_TARGET = _C['P3D_VIEW_HOLE'], _C['P3D_VIEW_CONSISTENT'], _C['P3D_VIEW_BEHIND'], _C['P3D_VIEW_IN_FRONT'], _C['P3D_VIEW_NO_TARGET']
STATUS_NAMES = ('hole', 'consistent', 'behind', 'in_front', 'no_target')
KEY_SCALE, KEY_LIMIT, GUARD = 65536.0, 2147483648.0, _C['P3D_VIEW_GUARD']      # zkey = floor(zc * 65536) < 2^31; a splat point may lie GUARD pixels outside the image
MAX_RADIUS, MAX_CHANNELS, MAX_FRAMES = _C['P3D_VIEW_MAX_RADIUS'], _C['P3D_VIEW_MAX_CHANNELS'], evaluate.MAX_FRAMES
MAX_TOLERANCE = _C['P3D_VIEW_MAX_TOLERANCE']
COUNT_LAUNCHES = {True: 5, False: 3}                         # consistency_counts: with labels / without


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
def _check_cameras(cameras, frames=None, what='cameras'):
    if not torch.is_tensor(cameras) or cameras.dtype != torch.float32 or cameras.ndim != 2 or cameras.shape[1] != 25:
        raise ValueError(f'{what} must be a float32 [F, 25] tensor of camera labels')
    if cameras.shape[0] > MAX_FRAMES or (frames is not None and cameras.shape[0] != frames):
        raise ValueError(f'{what}: {cameras.shape[0]} cameras for {frames} frames (at most {MAX_FRAMES})')
    return cameras.contiguous()


def _check_side(h, w, what):
    if not (1 <= h <= MAX_SIZE and 1 <= w <= MAX_SIZE):
        raise ValueError(f'{what}: a view is 1 .. {MAX_SIZE} pixels a side, got {h} x {w}')


def _check_points(points, frames, device, what='points', broadcast=True):
    """float32 [S, h, w, 3] (or [h, w, 3]: S = 1), every frame dense, S = ``frames`` or — ``broadcast`` — 1: (the view [S, h, w, 3], its frame pitch in floats)."""
    if not torch.is_tensor(points) or points.dtype != torch.float32 or points.ndim not in (3, 4) or points.shape[-1] != 3:
        raise ValueError(f'{what} must be a float32 [F, h, w, 3] tensor')
    p = points[None] if points.ndim == 3 else points
    s, h, w, _ = p.shape
    _check_side(h, w, what)
    if p.device != device or s not in ((1, frames) if broadcast else (frames,)):
        raise ValueError(f'{what} is {tuple(points.shape)} on {points.device}: {frames} frames (or one) on {device} are needed')
    if frames and p[0].stride() != (3 * w, 3, 1) and h * w > 1:
        raise ValueError(f'{what}: the points of a frame must be contiguous (strides {p.stride()})')
    pitch = 0 if (s == 1 and frames != 1) or (s > 1 and p.stride(0) == 0) else (p.stride(0) if s > 1 else 3 * h * w)
    if pitch != 0 and pitch < 3 * h * w:
        raise ValueError(f'{what}: frames overlap (strides {p.stride()})')
    return p, pitch


def _check_frames(t, name, frames, device, broadcast=False, channels=True):
    """uint8 / bool frames [h, w], [S, h, w] or — ``channels`` — [S, h, w, C] (C = 1 .. 4 interleaved) with contiguous pixels, rows and frames that do not
    overlap; S = ``frames`` or — ``broadcast`` — 1.  (the uint8 view [S, h, w, C], whether it had the channel dimension, row pitch, frame pitch in bytes)."""
    if not torch.is_tensor(t) or t.dtype not in (torch.uint8, torch.bool) or t.ndim not in ((2, 3, 4) if channels else (2, 3)):
        raise ValueError(f'{name} must be a uint8 [h, w], [F, h, w]{" or [F, h, w, C]" if channels else ""} tensor')
    had = t.ndim == 4
    v = t.view(torch.uint8) if t.dtype == torch.bool else t
    v = v[None, :, :, None] if v.ndim == 2 else (v[..., None] if v.ndim == 3 else v)
    s, h, w, c = v.shape
    _check_side(h, w, name)
    if not 1 <= c <= MAX_CHANNELS:
        raise ValueError(f'{name}: 1 .. {MAX_CHANNELS} interleaved channels, got {c}')
    if v.device != device or s not in ((1, frames) if broadcast else (frames,)):
        raise ValueError(f'{name} is {tuple(t.shape)} on {t.device}: {frames} frames{" (or one)" if broadcast else ""} on {device} are needed')
    row = v.stride(1) if h > 1 else w * c
    frame = 0 if (s == 1 and frames != 1) or (s > 1 and v.stride(0) == 0) else (v.stride(0) if s > 1 else h * row)
    if s and ((c > 1 and v.stride(3) != 1) or (w > 1 and v.stride(2) != c) or row < w * c or (frame != 0 and frame < (h - 1) * row + w * c)):
        raise ValueError(f'{name} must have contiguous pixels, rows and frames that do not overlap (strides {t.stride()})')
    return v, had, row, frame


def _check_int(value, lo, hi, what):
    if isinstance(value, bool) or value is None or int(value) != value or not lo <= int(value) <= hi:
        raise ValueError(f'{what} must be an integer {lo} .. {hi}, got {value!r}')
    return int(value)


def _check_zbuf(zbuf, what):
    if not torch.is_tensor(zbuf) or zbuf.dtype != torch.int64 or zbuf.ndim != 3 or not zbuf.is_contiguous() or zbuf.shape[0] > MAX_FRAMES:
        raise ValueError(f'{what} must be a contiguous int64 [F, H, W] tensor')
    _check_side(zbuf.shape[1], zbuf.shape[2], what)
    return tuple(zbuf.shape)


# ---- the projection: the definition ------------------------------------------------------------------------------------------------
def _project_torch(p, cameras, size):
    """The header's projection of ``p`` float32 [S, n, 3] (S = F or 1) under ``cameras`` [F, 25] into an H x W image, as fp64 element-wise ops in the header's
    order: (sx, sy, zs = zc * 65536 as float64 [F, n], ok bool [F, n]: finite, in front of the camera, below the key limit)."""
    h, w = size
    c = cameras.double()
    m = lambda k: c[:, k, None]
    qx, qy, qz = p[..., 0].double() - m(3), p[..., 1].double() - m(7), p[..., 2].double() - m(11)
    xc = m(0) * qx; xc = xc + m(4) * qy; xc = xc + m(8) * qz
    yc = m(1) * qx; yc = yc + m(5) * qy; yc = yc + m(9) * qz
    zc = m(2) * qx; zc = zc + m(6) * qy; zc = zc + m(10) * qz
    a = m(16) * xc; a = a + m(17) * yc
    u = a / zc + m(18)
    v = (m(20) * yc) / zc + m(21)
    zs = zc * KEY_SCALE
    ok = torch.isfinite(p).all(dim=-1) & (zc > 0) & (zs < KEY_LIMIT)
    return torch.floor(u * float(w)), torch.floor(v * float(h)), zs, ok


def points(depth, cameras):
    """float32 [F, h, w, 3]: the world points ``origins + depth * directions`` of the pixels of F views, rays from the project's own ``RaySampler`` (pixel
    centres, normalised directions: ``image_depth`` is the distance along them).  ``depth`` float32 [F, h, h] or [F, 1, h, h] (the sampler takes square
    views), ``cameras`` [F, 25].  Plain torch ops on either device: these are the kernels' INPUTS, no byte claim is made for them."""
    from .training.volumetric_rendering.ray_sampler import RaySampler
    cameras = _check_cameras(cameras)
    if not torch.is_tensor(depth) or depth.dtype != torch.float32 or depth.ndim not in (3, 4) or (depth.ndim == 4 and depth.shape[1] != 1):
        raise ValueError('points: depth must be a float32 [F, h, h] or [F, 1, h, h] tensor')
    f, h, w = depth.shape[0], depth.shape[-2], depth.shape[-1]
    if h != w or f != cameras.shape[0] or depth.device != cameras.device:
        raise ValueError(f'points: depth {tuple(depth.shape)} on {depth.device} for cameras {tuple(cameras.shape)} on {cameras.device}: square views, one per camera')
    origins, directions = RaySampler()(cameras[:, :16].view(-1, 4, 4), cameras[:, 16:25].view(-1, 3, 3), h)
    return (origins + depth.reshape(f, h * w, 1) * directions).view(f, h, w, 3)


# ---- splat -------------------------------------------------------------------------------------------------------------------------
def _splat_torch(p, cameras, valid, radius, zbuf):
    """``zbuf`` int64 [F, H, W] receives the minimum key per footprint pixel: one int64 ``scatter_reduce('amin')`` per footprint offset."""
    f, h, w = zbuf.shape
    n = p.shape[1]
    sx, sy, zs, ok = _project_torch(p, cameras, (h, w))
    keep = ok & (sx >= -GUARD) & (sx < w + GUARD) & (sy >= -GUARD) & (sy < h + GUARD)           # on the doubles, before any conversion
    if valid is not None:
        keep = keep & (valid.reshape(valid.shape[0], n) != 0)
    zero = torch.zeros((), dtype=torch.float64, device=p.device)
    ix, iy = torch.where(keep, sx, zero).long(), torch.where(keep, sy, zero).long()
    key = (torch.where(keep, torch.floor(zs), zero).long() << 32) + torch.arange(n, dtype=torch.int64, device=p.device)
    frame0 = torch.arange(f, dtype=torch.int64, device=p.device)[:, None] * (h * w)
    flat = zbuf.view(-1)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            tx, ty = ix + dx, iy + dy
            inside = keep & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            flat.scatter_reduce_(0, (frame0 + ty * w + tx)[inside], key[inside], 'amin', include_self=True)
    return zbuf


def splat(points, cameras, size=None, radius=0, valid=None, out=None):
    """int64 [F, H, W]: the z-buffer of the world points ``points`` (float32 [F, h, w, 3]; [1, h, w, 3] or [h, w, 3]: ONE source view seen by all F cameras)
    under ``cameras`` [F, 25] in views of ``size`` = (H, W) (default: the source's).  Every point i = y * w + x that is not dropped (p3d_regions.h: ``valid``
    byte 0, non-finite, not in front of the camera, zc >= 2^15, more than 4 pixels outside the image) puts ``key = floor(zc * 65536) * 2^32 + i`` on the pixels
    within ``radius`` (0, 1, 2: a square of 1, 9, 25 pixels) of its own, where the smallest key stays: the nearest point, the smallest index among equals.  ``out``: a
    buffer to splat into (default: a fresh one filled with ``EMPTY``); several sources may share one.  ``valid``: uint8 / bool [F, h, w] (or [h, w], [1, h, w]: one map
    for every frame), pitched views included.  Device tensors: ONE ``p3d_view_splat`` launch (none for F = 0), no host synchronisation; CPU tensors: the torch
    formulation, the definition."""
    cameras = _check_cameras(cameras)
    f, dev = cameras.shape[0], cameras.device
    p, pitch = _check_points(points, f, dev)
    h, w = p.shape[1:3]
    radius = _check_int(radius, 0, MAX_RADIUS, 'radius')
    big_h, big_w = (h, w) if size is None else (int(size[0]), int(size[1]))
    _check_side(big_h, big_w, 'size')
    v = v_row = v_frame = None
    if valid is not None:
        v, _, v_row, v_frame = _check_frames(valid, 'valid', f, dev, broadcast=True, channels=False)
        if tuple(v.shape[1:3]) != (h, w):
            raise ValueError(f'valid is {tuple(valid.shape)}, the points {tuple(points.shape)}: one byte per point')
    if out is None:
        out = torch.full([f, big_h, big_w], EMPTY, dtype=torch.int64, device=dev)
    elif _check_zbuf(out, 'out') != (f, big_h, big_w) or out.device != dev:
        raise ValueError(f'out must be a contiguous int64 [{f}, {big_h}, {big_w}] tensor on {dev}')
    if not out.is_cuda:
        return _splat_torch(p.reshape(p.shape[0], h * w, 3), cameras, None if v is None else v[..., 0], radius, out)
    with _lib.kernel_timer('view_splat', out):
        code = regions.regions_lib().p3d_view_splat(_lib.ptr(p), pitch, _lib.ptr(v), v_row or 0, v_frame or 0, _lib.ptr(cameras), f, h, w, radius,
                                                    _lib.ptr(out), big_h, big_w, _lib.stream_of(out))
    regions._check(code, 'view_splat')
    return out


# ---- resolve -----------------------------------------------------------------------------------------------------------------------
def _resolve_torch(zbuf, src, fill, target, cameras, tolerance):
    """(warped [F, H, W, C], status [F, H, W], index [F, H, W]) from ``src`` uint8 [S, h, w, C]."""
    f, h, w = zbuf.shape
    s, sh, sw, c = src.shape
    n = sh * sw
    i, zk = zbuf & 0xffffffff, zbuf >> 32
    hole = i >= n
    at = torch.where(hole, torch.zeros_like(i), i).view(f, h * w, 1).expand(-1, -1, c)
    carried = torch.gather(src.reshape(s, n, c).expand(f, n, c), 1, at).view(f, h, w, c)
    warped = torch.where(hole[..., None], torch.tensor(fill, dtype=torch.uint8, device=zbuf.device), carried)
    status = torch.ones_like(i)
    if target is not None:
        _, _, zs, ok = _project_torch(target.reshape(f, h * w, 3), cameras, (h, w))
        zt = torch.where(ok, torch.floor(zs), torch.zeros_like(zs)).long().view(f, h, w)
        status = torch.where((zk - zt).abs() <= tolerance, 1, torch.where(zk > zt, 2, 3))
        status = torch.where(ok.view(f, h, w), status, 4)
    status = torch.where(hole, 0, status)
    return warped, status.to(torch.uint8), torch.where(hole, -1, i).to(torch.int32)


def _fill_bytes(fill, c):
    values = [fill] * c if isinstance(fill, int) and not isinstance(fill, bool) else list(fill)
    if len(values) != c or any(isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 255 for v in values):
        raise ValueError(f'fill must be an integer 0 .. 255 or {c} of them, got {fill!r}')
    return [int(v) for v in values]


def resolve(zbuf, source, fill=0, target_points=None, cameras=None, tolerance=None, counts=None, return_index=False, out=None):
    """``(warped, status[, index])`` of a ``splat`` buffer ``zbuf`` int64 [F, H, W].  ``source``: the uint8 frames the points were lifted from, [F, h, w, C] with
    C = 1 .. 4 interleaved channels, [F, h, w] or [h, w] (one frame, or [1, ...]: ONE source for every camera), pitched views included.  Per target pixel with the
    key ``k``: a hole (``k == EMPTY``, or any index not below h * w) gets ``fill`` (an integer or C of them), index -1 and status ``HOLE``; otherwise
    ``warped = source[k & 0xffffffff]``, ``index`` (int32, with ``return_index``) that index and status ``CONSISTENT`` — or, with ``target_points`` (float32
    [F, H, W, 3]: the target views' own world points), ``cameras`` [F, 25] and ``tolerance`` (key units of 1 / 65536, 0 .. 2^31 - 1), with zt the key depth of the
    target's point under its camera: ``NO_TARGET`` (4) where that point is dropped, ``CONSISTENT`` (1) where ``|zk - zt| <= tolerance``, ``BEHIND`` (2) where
    ``zk > zt`` (the target sees a surface in front of the carried one: a disocclusion, not an error), ``IN_FRONT`` (3) otherwise (the source puts matter
    where the target sees through: an inconsistency).  ``warped`` has ``source``'s layout with H x W pixels (``out``: the caller's uint8 view of that shape, any
    row and frame pitch, not ``source``'s memory; bytes around it stay untouched); ``status`` is uint8 [F, H, W].  ``counts``: an int64 [5] counter that receives
    ``+= bincount(status)``.  Device tensors: ONE ``p3d_view_resolve`` launch (none for F = 0), no host synchronisation; CPU tensors:
    the torch formulation."""
    f, h, w = _check_zbuf(zbuf, 'zbuf')
    dev = zbuf.device
    src, had, s_row, s_frame = _check_frames(source, 'source', f, dev, broadcast=True)
    c = src.shape[3]
    fill = _fill_bytes(fill, c)
    target = None
    if target_points is not None:
        cameras = _check_cameras(cameras, f) if cameras is not None else None
        if cameras is None or cameras.device != dev:
            raise ValueError('resolve: target_points need the target cameras [F, 25] on the same device')
        tolerance = _check_int(tolerance, 0, MAX_TOLERANCE, 'tolerance')
        shaped = target_points.view(f, h, w, 3) if torch.is_tensor(target_points) and target_points.ndim == 3 and tuple(target_points.shape) == (f, h * w, 3) else target_points
        target, _ = _check_points(shaped, f, dev, 'target_points', broadcast=False)
        if tuple(target.shape) != (f, h, w, 3) or not target.is_contiguous():
            raise ValueError(f'target_points must be a contiguous float32 [{f}, {h}, {w}, 3] tensor, got {tuple(target_points.shape)}')
    elif cameras is not None or tolerance is not None:
        raise ValueError('resolve: cameras and tolerance go with target_points')
    if counts is not None:
        counts = evaluate._check_counter(counts, [5], dev, 'resolve')
    dst, d_row, d_frame = None, w * c, h * w * c
    if out is not None:
        if not torch.is_tensor(out) or tuple(out.shape) != ((f, h, w, c) if had else (f, h, w)) or out.dtype != torch.uint8:
            raise ValueError(f'resolve: out must be a uint8 {[f, h, w, c] if had else [f, h, w]} tensor')
        dst, _, d_row, d_frame = _check_frames(out, 'out', f, dev)
        if f and out.untyped_storage().data_ptr() == source.untyped_storage().data_ptr():
            raise ValueError('resolve writes out of place: out must not share memory with source')
    if not zbuf.is_cuda:
        warped, status, index = _resolve_torch(zbuf, src, fill, target, cameras, tolerance)
        if counts is not None:
            counts += torch.bincount(status.reshape(-1).long(), minlength=5)
        if dst is not None:
            dst.copy_(warped)
            warped = dst
    else:
        warped = torch.empty([f, h, w, c], dtype=torch.uint8, device=dev) if dst is None else dst
        status = torch.empty([f, h, w], dtype=torch.uint8, device=dev)
        index = torch.empty([f, h, w], dtype=torch.int32, device=dev) if return_index else None
        with _lib.kernel_timer('view_resolve', status):
            code = regions.regions_lib().p3d_view_resolve(_lib.ptr(zbuf), _lib.ptr(src), s_row, s_frame, src.shape[1], src.shape[2], c, (ctypes.c_uint8 * 4)(*fill),
                                                          _lib.ptr(warped), d_row, d_frame, _lib.ptr(index), _lib.ptr(status), _lib.ptr(target),
                                                          _lib.ptr(cameras) if target is not None else None, tolerance or 0, _lib.ptr(counts), f, h, w,
                                                          _lib.stream_of(status))
        regions._check(code, 'view_resolve')
    warped = out if out is not None else (warped if had else warped[..., 0])      # ([h, w] is one frame of one channel: [F, H, W] comes back)
    return (warped, status, index) if return_index else (warped, status)


# ---- difference histogram ----------------------------------------------------------------------------------------------------------
def _difference_histogram_torch(a, b, where, match):
    d = (a.to(torch.int16) - b.to(torch.int16)).abs()
    if where is not None:
        d = d[where[..., 0] == match]
    return torch.bincount(d.reshape(-1).long(), minlength=256)


def difference_histogram(a, b, where=None, match=1, out=None):
    """int64 [256]: ``hist[|a - b|] += 1`` per channel of every pixel with ``where == match`` (of every pixel: ``where`` None).  ``a`` / ``b``: uint8 [F, H, W, C]
    with C = 1 .. 4, [F, H, W] or [H, W], one shape, pitched views included; ``where``: uint8 / bool [F, H, W] (or [H, W]), e.g. ``resolve``'s status with
    ``match=CONSISTENT``.  ``out``: the caller's counter, accumulated into.  Device tensors: ONE ``p3d_view_difference_histogram`` launch (none for F = 0), no host
    synchronisation; CPU tensors: ``bincount``."""
    if not torch.is_tensor(a) or not torch.is_tensor(b) or tuple(a.shape) != tuple(b.shape) or a.ndim < 2:
        raise ValueError('difference_histogram: a and b must be uint8 tensors of one shape')
    f, dev = (1 if a.ndim == 2 else a.shape[0]), a.device
    va, _, a_row, a_frame = _check_frames(a, 'a', f, dev)
    vb, _, b_row, b_frame = _check_frames(b, 'b', f, dev)
    _, h, w, c = va.shape
    match = _check_int(match, 0, 255, 'match')
    vw, w_row, w_frame = None, 0, 0
    if where is not None:
        vw, _, w_row, w_frame = _check_frames(where, 'where', f, dev, channels=False)
        if tuple(vw.shape[:3]) != (f, h, w):
            raise ValueError(f'where is {tuple(where.shape)}, the frames {tuple(a.shape)}: one byte per pixel')
    out = evaluate._check_counter(out, [256], dev, 'difference_histogram')
    if not va.is_cuda:
        out += _difference_histogram_torch(va, vb, vw, match)
        return out
    with _lib.kernel_timer('view_difference_histogram', out):
        code = regions.regions_lib().p3d_view_difference_histogram(_lib.ptr(va), a_row, a_frame, _lib.ptr(vb), b_row, b_frame, _lib.ptr(vw), w_row, w_frame,
                                                                   match, c, f, h, w, _lib.ptr(out), _lib.stream_of(out))
    regions._check(code, 'view_difference_histogram')
    return out


# ---- compositions ------------------------------------------------------------------------------------------------------------------
def warp(source, depth, camera_from, cameras_to, radius=1, fill=0):
    """One rendered frame seen from other cameras — a novel-view preview without the generator: ``points`` -> ``splat`` -> ``resolve``.  ``source`` uint8 [h, h] or
    [h, h, C]; ``depth`` float32 [h, h] (distance along the pixel's ray, ``image_depth``); ``camera_from`` [25] or [1, 25]; ``cameras_to`` [F, 25].  Returns
    ``(warped [F, h, h(, C)], status [F, h, h])``: status ``HOLE`` where no point landed within ``radius``."""
    if not torch.is_tensor(source) or source.ndim not in (2, 3):
        raise ValueError('warp: source must be a uint8 [h, w] or [h, w, C] tensor')
    cameras_to = _check_cameras(cameras_to, what='cameras_to')
    pts = points(depth.reshape(1, *depth.shape[-2:]), camera_from.reshape(1, 25))
    zbuf = splat(pts, cameras_to, radius=radius)
    return resolve(zbuf, source[None], fill)


class Consistency:
    """Counters on ``device`` for a whole set of view pairs: ``status`` int64 [5], ``confusion`` int64 [C * C + 1] (C = ``n_labels``; 1 for generators without
    label maps, where it stays zero) and ``differences`` int64 [256].  ``add`` accumulates without a host synchronisation, ``result`` is the only read."""

    def __init__(self, n_labels, device):
        self.n_labels = None if n_labels is None else evaluate._check_labels(n_labels)
        cells = (self.n_labels or 1) ** 2 + 1
        self._store = torch.zeros([5 + cells + 256], dtype=torch.int64, device=device)           # one tensor: one copy to the host
        self.device = self._store.device                                        # ('cuda' becomes 'cuda:0': what the frames' tensors report)
        self.status, self.confusion, self.differences = self._store[:5], self._store[5:5 + cells], self._store[5 + cells:]
        self.pairs = 0                                                          # a host count of what was added

    def add(self, labels, images, depth, cameras, pairs, tolerance, radius=0):
        """``consistency_counts`` of the pairs into these counters."""
        consistency_counts(labels, images, depth, cameras, pairs, self.n_labels, tolerance, radius, out=self)

    def result(self):
        """``metrics_from_consistency`` of the counters so far (one copy to the host), with 'pairs' and 'n_labels'."""
        host = self._store.cpu()
        cells = self.confusion.numel()
        out = metrics_from_consistency(host[:5], host[5:5 + cells] if self.n_labels else None, host[5 + cells:])
        out.update(pairs=self.pairs, n_labels=self.n_labels)
        return out


def consistency_counts(labels, images, depth, cameras, pairs, n_labels, tolerance, radius=0, out=None):
    """The counters of a set of view pairs, as a ``Consistency`` (``out``: one to accumulate into).  ``labels`` uint8 [N, h, h] (None: a generator without label
    maps), ``images`` uint8 [N, h, h, C] (or [N, h, h]), ``depth`` float32 [N, h, h] and ``cameras`` [N, 25] are N views of one scene; ``pairs`` is a list of
    (i, j), i the source view and j the target view.  All pairs go through the kernels as one batch:

        zbuf = splat(points(depth, cameras)[i], cameras[j], radius)
        warped_labels, status = resolve(zbuf, labels[i], target_points=points[j], cameras=cameras[j], tolerance, counts=out.status)
        warped_images, _      = resolve(zbuf, images[i])
        evaluate.confusion(truth=labels[j], pred=warped_labels, n_labels, valid=status == CONSISTENT, out=out.confusion)
        difference_histogram(images[j], warped_images, status, CONSISTENT, out=out.differences)

    (without labels the one ``resolve`` of the images makes the status).  5 launches of libp3d_regions.so with labels, 3 without; no host synchronisation."""
    cameras = _check_cameras(cameras)
    n, dev = cameras.shape[0], cameras.device
    pairs = [(int(i), int(j)) for i, j in pairs]
    if any(not (0 <= i < n and 0 <= j < n) for i, j in pairs):
        raise ValueError(f'consistency_counts: pairs {pairs} of {n} views')
    tolerance = _check_int(tolerance, 0, MAX_TOLERANCE, 'tolerance')
    if out is None:
        out = Consistency(n_labels if labels is not None else None, dev)
    elif not isinstance(out, Consistency) or out.device != dev or out.n_labels != (n_labels if labels is not None else None):
        raise ValueError(f'consistency_counts: out must be a Consistency({n_labels}) on {dev}')
    if not pairs:
        return out
    pts = points(depth, cameras)
    source, target = [i for i, _ in pairs], [j for _, j in pairs]
    take = lambda t, which: torch.stack([t[k] for k in which])                  # python indices: no index tensor travels to the device
    cams, pts_to = take(cameras, target), take(pts, target)
    zbuf = splat(take(pts, source), cams, radius=radius)
    images = images if images.ndim == 4 else images[..., None]
    if labels is not None:
        warped_labels, status = resolve(zbuf, take(labels, source), 0, pts_to, cams, tolerance, counts=out.status)
        warped_images, _ = resolve(zbuf, take(images, source))
        evaluate.confusion(take(labels, target), warped_labels, out.n_labels, valid=status == CONSISTENT, out=out.confusion)
    else:
        warped_images, status = resolve(zbuf, take(images, source), 0, pts_to, cams, tolerance, counts=out.status)
    difference_histogram(take(images, target), warped_images, status, CONSISTENT, out=out.differences)
    out.pairs += len(pairs)
    return out


def metrics_from_consistency(status, confusion, differences):
    """The one host read of the three counters and their metrics, computed in float64 on the host; a plain dict.  With s = ``status`` (int64 [5]), n = sum(s),
    covered = n - s[0], h = ``differences`` (int64 [256]) and m = sum(h), every sum taken in bin order:

        pixels      n                                  covered     n - s[HOLE]
        coverage    covered / n                        (NaN for n = 0)
        consistent  s[CONSISTENT] / covered            behind      s[BEHIND] / covered           (disocclusions)
        in_front    s[IN_FRONT] / covered              the INCONSISTENCY RATE: the source puts matter where the target sees through
        no_target   s[NO_TARGET] / covered             (all four NaN for covered = 0)
        labels      ``evaluate.metrics_from_confusion(confusion)`` on the consistent pixels: cross-view 'accuracy', 'miou', ... (None without label maps)
        mad         sum_d d h[d] / m                   the mean absolute difference of the carried and the rendered bytes on the consistent pixels
        mse         sum_d d^2 h[d] / m                 psnr   10 log10(255^2 / mse)   (inf for mse = 0; all three NaN for m = 0)
        status_counts, differences                     the integer counters themselves, int64 CPU tensors"""
    for t, size, what in ((status, 5, 'status'), (differences, 256, 'differences')):
        if not torch.is_tensor(t) or t.dtype != torch.int64 or tuple(t.shape) != (size,):
            raise ValueError(f'metrics_from_consistency: {what} must be an int64 [{size}] tensor')
    s, h = status.cpu(), differences.cpu()
    counts, bins = s.tolist(), h.tolist()
    nan = float('nan')
    n = sum(counts)
    covered = n - counts[HOLE]
    share = lambda k: counts[k] / covered if covered else nan
    m = total = squares = 0
    for d in range(256):                                                        # in bin order: the integer sums are exact
        m += bins[d]
        total += d * bins[d]
        squares += d * d * bins[d]
    mse = squares / m if m else nan
    psnr = nan if not m else (float('inf') if squares == 0 else 10.0 * math.log10(255.0 * 255.0 / mse))
    return {'pixels': n, 'covered': covered, 'coverage': covered / n if n else nan, 'consistent': share(CONSISTENT), 'behind': share(BEHIND),
            'in_front': share(IN_FRONT), 'no_target': share(NO_TARGET), 'labels': None if confusion is None else evaluate.metrics_from_confusion(confusion),
            'mad': total / m if m else nan, 'mse': mse, 'psnr': psnr, 'status_counts': s.clone(), 'differences': h.clone()}


# ---- generators --------------------------------------------------------------------------------------------------------------------
def default_tolerance(G):
    """``round(65536 (ray_end - ray_start) / depth_resolution)``: one coarse sample spacing of the ray-marcher in key units — derived, not tuned."""
    rk = G.rendering_kwargs
    return int(round(KEY_SCALE * (float(rk['ray_end']) - float(rk['ray_start'])) / int(rk['depth_resolution'])))


def raw_frames(floats):
    """The views of a ``G.synthesis`` output dict at the NEURAL RENDERING resolution, where depth is defined, as ``consistency_counts`` takes them: a dict with
    'images' uint8 [N, h, h, 3] from ``image_raw`` (or, one label channel: [N, h, h, 4], the grey map of ``semantic_raw`` as the fourth channel), 'labels' uint8
    [N, h, h], the argmax of ``semantic_raw`` (None with fewer than two label channels), 'depth' float32 [N, h, h] and 'n_labels'.  ``views.frame_finish`` jobs:
    nothing leaves the device."""
    from . import mesh, views
    raw, depth = floats['image_raw'].float(), floats['image_depth'].float()
    n, _, h, w = raw.shape
    dev = raw.device
    sem = floats.get('semantic_raw')
    grey = sem is not None and sem.shape[1] == 1
    store = torch.empty([n, h, w, 4 if grey else 3], dtype=torch.uint8, device=dev)
    labels, jobs = None, []
    if grey:
        rgb, ink = torch.empty([n, h, w, 3], dtype=torch.uint8, device=dev), torch.empty([n, h, w], dtype=torch.uint8, device=dev)
        views.frame_finish([views.FrameJob(raw, rgb), views.FrameJob(sem.float(), ink)])
        store[..., :3], store[..., 3] = rgb, ink
    else:
        jobs.append(views.FrameJob(raw, store))
        if sem is not None and sem.shape[1] >= 2:
            labels, colours = torch.empty([n, h, w], dtype=torch.uint8, device=dev), torch.empty([n, h, w, 3], dtype=torch.uint8, device=dev)
            jobs.append(views.FrameJob(sem.float(), colours, views.LABEL, palette=mesh.default_palette(sem.shape[1]), dst_index=labels))
        views.frame_finish(jobs)
    return {'images': store, 'labels': labels, 'depth': depth.reshape(n, h, w), 'n_labels': None if labels is None else int(sem.shape[1])}


@torch.no_grad()
def video_consistency(G, ws, cfg='seg2cat', n_frames=16, stride=1, jitter='frozen', tolerance=None, radius=0, neural_rendering_resolution=None,
                      views_per_step=4, **synthesis_kwargs):
    """``Consistency.result()`` of the camera path of a video: ``views.video_cameras(G, cfg, n_frames)`` rendered by ``views.render_views(...,
    return_float=True)`` (ONE backbone pass), the frames made by ``raw_frames`` at the neural rendering resolution, and the pairs (k, k + stride), every
    frame warped into the camera ``stride`` frames on (``stride=0``: every frame into its own camera, which must give coverage 1 and nothing but consistent
    pixels).  ``tolerance`` defaults to ``default_tolerance(G)``, one coarse sample spacing; ``jitter='frozen'`` keeps the sampling noise equal between the
    frames.  For edge generators (one label channel) there is no label part: the grey map is the images' fourth channel.  The result also carries 'tolerance',
    'stride' and 'frames'."""
    from . import views
    stride, n_frames = _check_int(stride, 0, 1 << 20, 'stride'), _check_int(n_frames, 1, MAX_FRAMES, 'n_frames')
    cams = views.video_cameras(G, cfg, n_frames).to(ws.device)
    synthesis_kwargs.setdefault('noise_mode', 'const')
    nrr = views.VIDEO_CFG[cfg]['neural_rendering_resolution'] if neural_rendering_resolution is None else neural_rendering_resolution
    rendered = views.render_views(G, ws, cams, views_per_step=views_per_step, jitter=jitter, neural_rendering_resolution=nrr, return_float=True, **synthesis_kwargs)
    frames = raw_frames(rendered['float'])
    tolerance = default_tolerance(G) if tolerance is None else tolerance
    pairs = [(k, k + stride) for k in range(n_frames - stride)]
    total = consistency_counts(frames['labels'], frames['images'], frames['depth'], cams, pairs, frames['n_labels'], tolerance, radius)
    out = total.result()
    out.update(tolerance=int(tolerance), stride=stride, frames=n_frames)
    return out


def turned_camera(camera, pivot, yaw=0.0, pitch=0.0, roll=0.0):
    """float32 [1, 25]: ``camera`` ([25] or [1, 25]) turned about the world point ``pivot`` by Ry(yaw) Rx(pitch) Rz(roll), radians — a rigid motion, so a camera
    that looks at the pivot still does; the intrinsics stay.  Computed in float64 on the host (one read of the label)."""
    label = camera.detach().reshape(25).cpu().double().numpy()
    a, b, c = float(yaw), float(pitch), float(roll)
    ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    turn, p = np.eye(4), np.asarray(pivot, dtype=np.float64).reshape(3)
    turn[:3, :3] = ry @ rx @ rz
    turn[:3, 3] = p - turn[:3, :3] @ p
    label[:16] = (turn @ label[:16].reshape(4, 4)).reshape(16)
    return torch.from_numpy(label).to(torch.float32).reshape(1, 25).to(camera.device)
