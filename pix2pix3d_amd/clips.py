"""What every caller of libp3d_video.so shares: the library, its header, and the clip contract of its entry points.

The frame writers (``video/``) and the frame measures (``quality.py``) call one kernel library (csrc/video/p3d_video.h states its rules).  Their clips are
uint8 [F, H, W, bpp] — [F, H, W] for one byte a pixel — with contiguous pixels and any row and frame pitch, and every entry point that reads a clip begins
with the same six arguments: ``check_frames`` is that contract, ``clip_args`` builds those arguments.  Nothing else of the package is imported here."""
import torch

from . import _lib

_side = _lib.SideLibrary('video')                    # libp3d_video.so: loaded on the first call, device-guarded; launch_count() is its own counter
VIDEO_LIB_PATH, HEADER = _side.path, _side.header
video_lib, launch_count, check = _side.lib, _side.launch_count, _side.check
MAX_PIXELS = 1 << 31                                 # F * H * W stays below it


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
