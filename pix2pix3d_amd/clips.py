"""What every caller of libp3d_video.so shares: the library, its header, and the clip contract of its entry points.

The frame writers and readers (``video/``), the frame measures (``quality.py``, ``multiscale.py``) and the resampler (``resample.py``) call one kernel
library, the one of everything that works on uint8 clips (csrc/video/p3d_video.h states its rules).  Their clips are uint8 [F, H, W, bpp] — [F, H, W] for
one byte a pixel — with contiguous pixels and any row and frame pitch, and every entry point that reads a clip begins with the same six arguments:
``check_frames`` is that contract, ``clip_args`` builds those arguments.  The checks that more than one of those modules makes stand here too:
``check_pair`` (two clips of one shape on one device) with ``pair_args``, ``check_sums`` (an int64 accumulator) and ``check_out`` (a destination clip
apart from its source).  Nothing else of the package is imported here."""
import torch

from . import _lib

_side = _lib.SideLibrary('video')                    # libp3d_video.so: loaded on the first call, device-guarded; launch_count() is its own counter
VIDEO_LIB_PATH, HEADER = _side.path, _side.header
video_lib, launch_count, check = _side.lib, _side.launch_count, _side.check
MAX_PIXELS = 1 << 31                                 # F * H * W stays below it
ANY_BPP = (1, 2, 3, 4)


def check_frames(frames, what='frames', bpp=(3,)):
    """(F, H, W) of uint8 [F, H, W, 3] frames with contiguous pixels and fewer than 2^31 of them; ValueError otherwise.  ``bpp``: the bytes a pixel may
    have — [F, H, W, bpp], and [F, H, W] for 1 — with fewer than 2^31 bytes (the PNG stages)."""
    shape = ' or '.join('[F, H, W]' if b == 1 else f'[F, H, W, {b}]' for b in bpp)
    ok = torch.is_tensor(frames) and frames.dtype == torch.uint8
    if not ok or not ((frames.ndim == 4 and frames.shape[3] in bpp and frames.shape[3] > 1) or (frames.ndim == 3 and 1 in bpp)):
        raise ValueError(f'{what} must be a uint8 {shape} tensor, got '
                         f'{str(frames.dtype) + " " + str(tuple(frames.shape)) if torch.is_tensor(frames) else type(frames).__name__}')
    f, h, w = frames.shape[:3]
    b = frames.shape[3] if frames.ndim == 4 else 1
    if f * h * w * (b if tuple(bpp) != (3,) else 1) >= MAX_PIXELS:
        raise ValueError(f'{what}: {f} x {h} x {w} pixels reach 2^31')
    strides = tuple(frames.stride()) + (1,) * (4 - frames.ndim)
    if f * h * w and (strides[3] != 1 or strides[2] != b or strides[1] < b * w or strides[0] < 0):
        raise ValueError(f'{what}: pixels must be contiguous (strides [*, >= {b * w}, {b}, 1]), got strides {tuple(frames.stride())}')
    return f, h, w


def clip_args(frames):
    """The leading arguments of every entry point."""
    f, h, w = frames.shape[:3]
    return _lib.ptr(frames), frames.stride(0), frames.stride(1), f, h, w


def bpp_of(frames):
    """The bytes of a pixel: 1 for [F, H, W]."""
    return frames.shape[3] if frames.ndim == 4 else 1


def channels(frames):
    """The clip as [F, H, W, bpp], a view: [F, H, W] gains its one channel."""
    return frames if frames.ndim == 4 else frames[..., None]


def check_pair(a, b, what):
    """(F, H, W, bpp) of two clips of one shape on one device."""
    f, h, w = check_frames(a, f'{what}: a', bpp=ANY_BPP)
    check_frames(b, f'{what}: b', bpp=ANY_BPP)
    if a.shape != b.shape:
        raise ValueError(f'{what}: a is {tuple(a.shape)}, b is {tuple(b.shape)}')
    if a.device != b.device:
        raise ValueError(f'{what}: a is on {a.device}, b on {b.device}')
    return f, h, w, bpp_of(a)


def pair_args(a, b):
    """The leading arguments of the entry points on two clips: both with their pitches, then F, H, W, bpp."""
    f, h, w = a.shape[:3]
    return _lib.ptr(a), a.stride(0), a.stride(1), _lib.ptr(b), b.stride(0), b.stride(1), f, h, w, bpp_of(a)


def check_sums(out, shape, device, what):
    """The int64 accumulator of a measure: the caller's contiguous ``out`` of ``shape`` on ``device``, or a zeroed one."""
    if out is None:
        return torch.zeros(shape, dtype=torch.int64, device=device)
    if not torch.is_tensor(out) or out.dtype != torch.int64 or tuple(out.shape) != tuple(shape) or out.device != device or not out.is_contiguous():
        raise ValueError(f'{what}: out must be a contiguous int64 {list(shape)} tensor on {device}')
    return out


def _byte_span(t):
    first = t.data_ptr()
    return first, first + sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1


def check_out(out, shape, frames, who):
    """The destination clip of ``shape`` for a result made from ``frames``: the caller's ``out`` — any row and frame pitch, its frames apart from each
    other and its bytes apart from the source's — or a new contiguous one."""
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=frames.device)
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or out.device != frames.device:
        raise ValueError(f'{who}: out must be uint8 {tuple(shape)} on {frames.device}')
    check_frames(out, 'out', bpp=ANY_BPP)
    if out.numel() and frames.numel():
        if out.ndim > 1 and shape[0] > 1 and out.stride(0) < (shape[1] - 1) * out.stride(1) + shape[2] * (shape[3] if len(shape) == 4 else 1):
            raise ValueError(f'{who}: the frames of out overlap each other (strides {tuple(out.stride())})')
        lo, hi = _byte_span(out)
        f_lo, f_hi = _byte_span(frames)
        if lo < f_hi and f_lo < hi:
            raise ValueError(f'{who} writes out of place: the bytes out spans must not meet the frames\'')
    return out
