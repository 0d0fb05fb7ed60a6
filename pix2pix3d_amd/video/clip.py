"""One writer for a clip: the choice among the frame writers that ``views.generate_video`` and ``surface.geometry_video`` offer, made in one place."""
import torch

from .avi import save_avi
from .gif import save_gif, save_gif_indexed
from .jpeg import jpeg_quality_for
from .png import save_apng


def check_clip_options(who, gif, format, psnr, ssim, ms_ssim=None):
    """ValueError, in ``who``'s name, for options no writer serves: a caller checks before it renders."""
    if gif not in ('pil', 'device'):
        raise ValueError(f"{who}: gif must be 'pil' or 'device', got {gif!r}")
    if format not in ('gif', 'avi', 'apng'):
        raise ValueError(f"{who}: format must be 'gif', 'avi' or 'apng', got {format!r}")
    if (psnr is not None or ssim is not None or ms_ssim is not None) and format != 'avi':
        raise ValueError(f"{who}: psnr / ssim / ms_ssim pick a JPEG quality and need format='avi', got {format!r}")


def save_clip(path, frames, fps=60, format='gif', gif='pil', psnr=None, ssim=None, indices=None, palette=None, who='save_clip', ms_ssim=None):
    """uint8 frames [F, H, W, 3], or grey [F, H, W], on the device or the host, written to ``path``.  ``format='avi'``: a Motion-JPEG AVI (``save_avi``; grey
    frames as three equal channels; ``gif`` plays no part) — at the default quality or, with ``psnr``, ``ssim`` or ``ms_ssim`` (one of them), at the quality that
    ``jpeg_quality_for`` picks for that target, whose ``(quality, metrics, met)`` is returned.  ``format='apng'``: a lossless animated PNG (``save_apng``).
    ``format='gif'``: ``gif='device'`` through ``save_gif`` (one palette for the clip, made and applied where the frames are; grey frames losslessly with a
    grey ramp), ``gif='pil'`` through ``mesh.save_gif``, PIL quantising every frame on the host.  ``indices`` uint8 [F, H, W] with their ``palette``
    uint8 [K, 3]: the same clip as palette indices, which the APNG and the device GIF store losslessly in place of ``frames``; the other writers take
    ``frames``.  Returns None but for an AVI with a target."""
    check_clip_options(who, gif, format, psnr, ssim, ms_ssim)
    if format == 'avi':
        if frames.ndim == 3:
            frames = frames[..., None].expand(-1, -1, -1, 3).contiguous()
        if psnr is None and ssim is None and ms_ssim is None:
            save_avi(path, frames, fps=fps)
            return None
        q = jpeg_quality_for(frames, psnr, ssim, ms_ssim=ms_ssim)
        save_avi(path, frames, fps=fps, quality=q[0])
        return q
    if format == 'apng':
        if indices is not None:
            save_apng(path, indices, fps=fps, mode='P', palette=palette)
        else:
            save_apng(path, frames, fps=fps)
    elif gif == 'device':
        if indices is not None:
            save_gif_indexed(path, indices, palette, fps=fps)
        elif frames.ndim == 3:
            save_gif_indexed(path, frames, torch.arange(256, dtype=torch.uint8)[:, None].expand(256, 3), fps=fps)
        else:
            save_gif(path, frames, fps=fps)
    else:
        from .. import mesh
        mesh.save_gif(path, frames.cpu().numpy(), fps=fps)
    return None
