"""Many views of one latent, and displayable frames without leaving the device: the native form of the reference's
``applications/generate_video.py`` and ``applications/generate_samples.py`` after their inputs.

The scripts render a video by calling ``G.synthesis(ws, pose)`` once per frame — the tri-plane backbone runs again for every frame to
produce the same planes — and finish every frame on the host in numpy after a synchronising copy (generate_video.py:54-99).  Here the
backbone runs ONCE (``G.backbone_planes``), the views go through the ray-marcher in chunks of ``views_per_step`` cameras over that one
plane set (the shared-plane launch of ``renderer.fused_render``) and through the generator's own super-resolution heads, and every
chunk is turned into uint8 frames by one launch of ``p3d_frame_finish`` (csrc/frame_ops.hip).

    cams = views.video_cameras(G, 'seg2cat')                       # float32 [120, 25]
    out = views.render_views(G, ws, cams.to(ws.device), noise_mode='const', neural_rendering_resolution=128)
    out['image'], out['label'], out['label_index']                 # uint8 [120,512,512,3], [120,512,512,3], [120,512,512] on ws.device
    views.generate_video(G, ws, 'seg2cat', 'cat.gif', 'cat_label.gif')

Finishing rules (identical bytes on the device kernel and in the torch formulation CPU tensors take):
  SCALE  u8 = (uint8)clamp((x - lo) * s, 0, 255) in fp32, difference and product rounded separately, truncation toward zero, NaN -> 0,
         s = 255 / (hi - lo) rounded once to fp32.  lo, hi = -1, 1 is both formulas of the scripts, ``(clip(x, -1, 1) + 1) * 127.5``
         (generate_video.py:65) and ``clip((x + 1) * 127.5, 0, 255)`` (:81-82; generate_samples.py:116-120).
  LABEL  k = argmax over the label channels by ``torch.argmax``'s CPU rules (first maximal channel; a NaN is the maximum, the first
         NaN wins), coloured by ``palette[k]`` (``training/utils.py:5-15`` with the caller's palette; default ``mesh.default_palette``).
"""
import contextlib
import ctypes
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib, mesh
from . import resample as rs                       # (``resample`` is the name of the scripts' filter argument)
from .training.volumetric_rendering import renderer as rmod

SCALE, LABEL = _lib.P3D_FRAME_SCALE, _lib.P3D_FRAME_LABEL
MAX_JOBS = _lib.P3D_FRAME_MAX_JOBS
_FrameJobC = _lib.p3d_frame_job         # the struct class, derived from include/p3d_hip.h


class FrameJob(NamedTuple):
    """One conversion of ``frame_finish``: ``src`` float32 [n, c, h, w] (any strides) -> the rectangle at (x0, y0) of ``dst`` uint8
    [n, H, W, 3] or [n, H, W] (pixels contiguous; rows and frames may be views of a larger canvas)."""
    src: torch.Tensor
    dst: torch.Tensor
    mode: int = SCALE
    lo: float = -1.0
    hi: float = 1.0
    palette: Optional[torch.Tensor] = None          # LABEL: uint8 [c, 3]; a CPU tensor travels by value, a device tensor is read in place
    dst_index: Optional[torch.Tensor] = None        # LABEL: uint8 [n, H, W], receives k
    x0: int = 0
    y0: int = 0


def scale_factor(lo, hi):
    """255 / (hi - lo), rounded once to fp32 (what both the kernel and the torch formulation multiply by)."""
    return float(np.float32(255.0 / (float(hi) - float(lo))))


def _check_job(j):
    src, dst = j.src, j.dst
    if src.dtype != torch.float32 or src.ndim != 4:
        raise ValueError(f'frame_finish: src must be float32 [n, c, h, w], got {src.dtype} {tuple(src.shape)}')
    n, c, h, w = src.shape
    bpp = 3 if dst.ndim == 4 else 1
    if dst.dtype != torch.uint8 or dst.ndim not in (3, 4) or (dst.ndim == 4 and (dst.shape[3] != 3 or dst.stride(3) != 1)) or dst.stride(2) != bpp:
        raise ValueError(f'frame_finish: dst must be uint8 [n, H, W, 3] or [n, H, W] with contiguous pixels, got {dst.dtype} {tuple(dst.shape)} strides {dst.stride()}')
    if dst.device != src.device or dst.shape[0] != n or j.x0 < 0 or j.y0 < 0 or j.y0 + h > dst.shape[1] or j.x0 + w > dst.shape[2]:
        raise ValueError(f'frame_finish: the {n} x {h} x {w} rectangle at ({j.x0}, {j.y0}) does not fit dst {tuple(dst.shape)} on {dst.device}')
    if min(n, h, w) < 1 or any(s < 0 for s in src.stride()) or any(s < 0 for s in dst.stride()):
        raise ValueError('frame_finish: empty tensors and negative strides are not supported')
    if j.mode == SCALE:
        if c not in (1, 3) or c != bpp or j.dst_index is not None:
            raise ValueError(f'frame_finish: SCALE writes c = 1 -> [n, H, W] or c = 3 -> [n, H, W, 3] (c = {c}, dst {tuple(dst.shape)})')
        if not float(j.hi) > float(j.lo):
            raise ValueError('frame_finish: SCALE needs hi > lo')
    elif j.mode == LABEL:
        if not 2 <= c <= 64 or bpp != 3:
            raise ValueError(f'frame_finish: LABEL takes 2 .. 64 channels and a [n, H, W, 3] destination (c = {c}, dst {tuple(dst.shape)})')
        pal = j.palette
        if pal is None or pal.dtype != torch.uint8 or tuple(pal.shape) != (c, 3):
            raise ValueError(f'frame_finish: LABEL needs a uint8 [{c}, 3] palette')
        k = j.dst_index
        if k is not None and (k.dtype != torch.uint8 or k.ndim != 3 or k.stride(2) != 1 or k.device != src.device or k.shape[0] != n
                              or j.y0 + h > k.shape[1] or j.x0 + w > k.shape[2] or any(s < 0 for s in k.stride())):
            raise ValueError(f'frame_finish: dst_index must be uint8 [n, H, W] holding the rectangle, got {k.dtype} {tuple(k.shape)}')
    else:
        raise ValueError(f'frame_finish: unknown mode {j.mode}')
    return n, c, h, w, bpp


def _finish_cpu(j, n, c, h, w):
    """The torch formulation (identical bytes)."""
    ys, xs = slice(j.y0, j.y0 + h), slice(j.x0, j.x0 + w)
    if j.mode == SCALE:
        lo, s = torch.tensor(j.lo, dtype=torch.float32), torch.tensor(scale_factor(j.lo, j.hi), dtype=torch.float32)
        t = (j.src - lo) * s                                             # two fp32 roundings
        u8 = torch.where(t > 0, t.clamp(max=255.0), torch.zeros_like(t)).to(torch.uint8)          # NaN fails the comparison -> 0; truncation
        if c == 3:
            j.dst[:, ys, xs, :] = u8.permute(0, 2, 3, 1)
        else:
            j.dst[:, ys, xs] = u8[:, 0]
        return
    k = torch.argmax(j.src, dim=1)
    j.dst[:, ys, xs, :] = j.palette.to(j.src.device)[k]
    if j.dst_index is not None:
        j.dst_index[:, ys, xs] = k.to(torch.uint8)


def frame_finish(jobs):
    """Run the conversions ``jobs`` (a list of ``FrameJob``): device tensors by ``p3d_frame_finish``, at most ``MAX_JOBS`` per launch and nothing
    else on the stream (no allocation, no copy); CPU tensors by the torch formulation with the same bytes."""
    jobs = list(jobs)
    shapes = [_check_job(j) for j in jobs]
    if not jobs:
        return
    if any(j.src.device != jobs[0].src.device for j in jobs):
        raise ValueError('frame_finish: the jobs of one call live on one device')
    if not jobs[0].src.is_cuda:
        for j, (n, c, h, w, _) in zip(jobs, shapes):
            _finish_cpu(j, n, c, h, w)
        return
    lib = _lib.lib()
    keep = []
    for head in range(0, len(jobs), MAX_JOBS):
        part = list(zip(jobs[head:head + MAX_JOBS], shapes[head:head + MAX_JOBS]))
        arr = (_FrameJobC * len(part))()
        for q, (j, (n, c, h, w, bpp)) in zip(arr, part):
            q.src, q.src_stride = j.src.data_ptr(), (ctypes.c_int64 * 4)(*j.src.stride())
            q.dst, q.dst_row_pitch, q.dst_frame_pitch = j.dst.data_ptr(), j.dst.stride(1), j.dst.stride(0)
            if j.dst_index is not None:
                q.dst_index, q.index_row_pitch, q.index_frame_pitch = j.dst_index.data_ptr(), j.dst_index.stride(1), j.dst_index.stride(0)
            q.mode, q.n, q.c, q.h, q.w, q.x0, q.y0, q.dst_bpp = j.mode, n, c, h, w, j.x0, j.y0, bpp
            if j.mode == SCALE:
                q.lo, q.scale = float(j.lo), scale_factor(j.lo, j.hi)
            elif j.palette.is_cuda:
                pal = j.palette.contiguous()
                keep.append(pal)
                q.palette_dev = pal.data_ptr()
            else:
                ctypes.memmove(q.palette, j.palette.contiguous().data_ptr(), 3 * c)
        t = part[0][0].dst
        with _lib.kernel_timer('frame_finish', t):
            code = lib.p3d_frame_finish(ctypes.cast(arr, ctypes.c_void_p), len(part), _lib.stream_of(t))
        _lib.check(code, 'frame_finish')


# ---- one output dictionary -> frames ----------------------------------------------------------------------------------------
def _frame_jobs(out, dst, palette, depth_range):
    """The jobs that turn one ``G.synthesis`` output dict into the frames ``dst`` (a dict of uint8 tensors made by ``_alloc_frames``)."""
    jobs = [FrameJob(out['image'].float(), dst['image'])]
    if 'label' in dst:
        sem = out['semantic'].float()
        if dst['label'].ndim == 3:                                      # grey, as the scripts write edge maps: channel 0 of the label head
            jobs.append(FrameJob(sem[:, :1], dst['label']))
        else:
            jobs.append(FrameJob(sem, dst['label'], LABEL, palette=palette, dst_index=dst['label_index']))
    if 'depth' in dst:
        jobs.append(FrameJob(out['image_depth'].float(), dst['depth'], SCALE, float(depth_range[0]), float(depth_range[1])))
    return jobs


def _label_layout(out, label_mode):
    if 'semantic' not in out:
        return None
    c = out['semantic'].shape[1]
    if label_mode == 'auto':
        label_mode = 'grey' if c == 1 else 'palette'
    if label_mode not in ('grey', 'palette') or (label_mode == 'palette' and c < 2):
        raise ValueError(f"label_mode must be 'auto', 'palette' (two or more label channels) or 'grey', got {label_mode!r} for {c} channels")
    return label_mode


def _alloc_frames(out, n_frames, depth_range, label_mode):
    dev = out['image'].device
    h, w = out['image'].shape[-2:]
    dst = {'image': torch.empty([n_frames, h, w, 3], dtype=torch.uint8, device=dev)}
    mode = _label_layout(out, label_mode)
    if mode is not None:
        hs, wsz = out['semantic'].shape[-2:]
        if mode == 'grey':
            dst['label'] = torch.empty([n_frames, hs, wsz], dtype=torch.uint8, device=dev)
        else:
            dst['label'] = torch.empty([n_frames, hs, wsz, 3], dtype=torch.uint8, device=dev)
            dst['label_index'] = torch.empty([n_frames, hs, wsz], dtype=torch.uint8, device=dev)
    if depth_range is not None:
        hd, wd = out['image_depth'].shape[-2:]
        dst['depth'] = torch.empty([n_frames, hd, wd], dtype=torch.uint8, device=dev)
    return dst


def _palette_for(out, palette):
    if 'semantic' not in out or out['semantic'].shape[1] < 2:
        return None
    c = out['semantic'].shape[1]
    pal = mesh.default_palette(c) if palette is None else torch.as_tensor(palette)
    if pal.dtype != torch.uint8 or tuple(pal.shape) != (c, 3):
        raise ValueError(f'palette must be uint8 [{c}, 3], got {pal.dtype} {tuple(pal.shape)}')
    return pal


@torch.no_grad()
def finish_frames(out, palette=None, depth_range=None, label_mode='auto'):
    """The numpy finishing of one ``G.synthesis`` output dict (generate_samples.py:116-120, the demo, the snapshot grids), on the tensors' device:
    ``image`` uint8 [N,H,W,3]; with label channels ``label`` uint8 [N,H,W,3] (palette colours of the argmax) and ``label_index`` uint8 [N,H,W], or —
    one label channel / ``label_mode='grey'`` — ``label`` uint8 [N,H,W] grey; with ``depth_range=(near, far)`` also ``depth`` uint8 [N,h,w]."""
    dst = _alloc_frames(out, out['image'].shape[0], depth_range, label_mode)
    frame_finish(_frame_jobs(out, dst, _palette_for(out, palette), depth_range))
    return dst


# ---- cameras ----------------------------------------------------------------------------------------------------------------
# generate_video.py:120-139 per --cfg.  main() renders BOTH edge configurations with render_video_edge2cat (yaw0 = +3.14/2, yaw on the sine: the seg
# turntable), never render_video_edge; edge2cat also takes the seg branch's ranges, focal length and 128^2 rays.
VIDEO_CFG = {
    'seg2cat': dict(pitch_range=0.25, yaw_range=0.35, focal=4.2647, neural_rendering_resolution=128),
    'seg2face': dict(pitch_range=0.25, yaw_range=0.35, focal=4.2647, neural_rendering_resolution=128),
    'edge2cat': dict(pitch_range=0.25, yaw_range=0.35, focal=4.2647, neural_rendering_resolution=128),
    'edge2car': dict(pitch_range=np.pi / 2, yaw_range=np.pi, focal=1.7074, neural_rendering_resolution=64),
}


def camera_labels(cam2world, intrinsics):
    """float32 [F, 25] camera labels ``cat(cam2world.reshape(-1, 16), intrinsics.reshape(-1, 9))`` from cam2world [F, 4, 4] (or [4, 4]) and
    intrinsics [3, 3] (shared) or [F, 3, 3]."""
    c2w = torch.as_tensor(cam2world, dtype=torch.float32).reshape(-1, 16)
    k = torch.as_tensor(intrinsics, dtype=torch.float32).reshape(-1, 9).to(c2w.device)
    if k.shape[0] not in (1, c2w.shape[0]):
        raise ValueError(f'camera_labels: {c2w.shape[0]} poses with {k.shape[0]} intrinsics')
    return torch.cat([c2w, k.expand(c2w.shape[0], -1)], dim=1)


def video_cameras(G, cfg='seg2cat', n_frames=120):
    """float32 [n_frames, 25]: the camera labels generate_video.py renders for ``--cfg`` (see ``VIDEO_CFG``) about
    ``G.rendering_kwargs['avg_camera_pivot']`` at ``['avg_camera_radius']``."""
    if cfg not in VIDEO_CFG:
        raise ValueError(f'video_cameras: cfg must be one of {sorted(VIDEO_CFG)}, got {cfg!r}')
    v, rk = VIDEO_CFG[cfg], G.rendering_kwargs
    poses = mesh.turntable_poses(rk['avg_camera_pivot'], rk['avg_camera_radius'], n_frames, yaw_range=v['yaw_range'], pitch_range=v['pitch_range'])
    f = v['focal']
    return camera_labels(poses, torch.tensor([[f, 0, 0.5], [0, f, 0.5], [0, 0, 1]], dtype=torch.float32))


# ---- many views ---------------------------------------------------------------------------------------------------------------
_frozen_draws = rmod._replay_draws      # (one chunk's draws: logical [n, M, Sc, 1] / [n * M, Sf], whichever way a route asks for them)


@torch.no_grad()
def render_views(G, ws, cameras, views_per_step=4, jitter='random', neural_rendering_resolution=None, return_float=False, palette=None,
                 depth_range=None, label_mode=None, **synthesis_kwargs):
    """The ``for frame_idx`` loop of generate_video.py's ``render_video*``: F cameras (float32 [F, 25]) of the latent ``ws`` [1, num_ws, w_dim].

    The backbone runs once; the views are rendered ``views_per_step`` at a time over that one plane set (``G.synthesis(..., use_cached_backbone=True)``
    on planes of batch 1: one ray-marcher launch per chunk, the depth clamp that of a batch of ``views_per_step``) and finished on the device.
    ``ws`` [F, num_ws, w_dim] (a latent per frame) is accepted and takes the ordinary equal-batch route per chunk.

    jitter   'random': every chunk draws its stratified / importance uniforms as a batch would (the reference's behaviour).
             'frozen': ONE view's uniforms are drawn before anything else (``torch.rand([1, M, Sc, 1])`` then ``torch.rand([M, Sf])`` on ws.device) and reused by
             every view and chunk: no shimmer between frames, and results do not depend on ``views_per_step``.  A tuple ``(u_coarse [1, M, Sc, 1], u_fine [M, Sf])``
             is 'frozen' with the caller's draws.
    Returns a dict of tensors on ws.device: ``image`` uint8 [F,H,W,3]; for label generators ``label`` uint8 [F,H,W,3] + ``label_index`` uint8 [F,H,W]
    (``G.data_type == 'edge'`` or one label channel: ``label`` uint8 [F,H,W] grey); ``depth`` uint8 [F,h,w] with ``depth_range=(near, far)``; with
    ``return_float`` also ``float``: the dict of float tensors (``image``, ``semantic``, ``image_depth``, ...) the frames were made from, all F views.
    ``G._last_planes`` (the ``cache_backbone`` slot) is left as it was found."""
    if not hasattr(G, 'backbone_planes') or not hasattr(G, '_last_planes'):
        raise TypeError(f'render_views: {type(G).__name__} is not built on the one-backbone tri-plane core')
    cameras = torch.as_tensor(cameras, dtype=torch.float32).to(ws.device)
    if cameras.ndim != 2 or cameras.shape[1] != 25 or ws.ndim != 3:
        raise ValueError(f'render_views: cameras must be [F, 25] and ws [1 or F, num_ws, w_dim], got {tuple(cameras.shape)} and {tuple(ws.shape)}')
    n_frames, step = cameras.shape[0], int(views_per_step)
    if step < 1 or n_frames < 1 or ws.shape[0] not in (1, n_frames):
        raise ValueError(f'render_views: {n_frames} cameras, views_per_step {step}, {ws.shape[0]} latents')
    per_frame = ws.shape[0] != 1
    if label_mode is None:
        label_mode = 'grey' if getattr(G, 'data_type', None) == 'edge' else 'auto'
    nrr = G.neural_rendering_resolution if neural_rendering_resolution is None else int(neural_rendering_resolution)
    rk = G.rendering_kwargs
    frozen = None
    if isinstance(jitter, (tuple, list)):
        frozen = tuple(torch.as_tensor(u, dtype=torch.float32).to(ws.device) for u in jitter)
    elif jitter == 'frozen':
        frozen = (torch.rand([1, nrr * nrr, int(rk['depth_resolution']), 1], device=ws.device), torch.rand([nrr * nrr, int(rk['depth_resolution_importance'])], device=ws.device))
    elif jitter != 'random':
        raise ValueError(f"render_views: jitter must be 'random', 'frozen' or a pair of draws, got {jitter!r}")
    if frozen is not None and (tuple(frozen[0].shape) != (1, nrr * nrr, int(rk['depth_resolution']), 1) or tuple(frozen[1].shape) != (nrr * nrr, int(rk['depth_resolution_importance']))):
        raise ValueError(f'render_views: frozen draws must be [1, {nrr * nrr}, {rk["depth_resolution"]}, 1] and [{nrr * nrr}, {rk["depth_resolution_importance"]}]')

    planes = None if per_frame else G.backbone_planes(ws, **synthesis_kwargs)
    found = G._last_planes
    dst, pal, floats = None, None, {}
    try:
        if frozen is not None and not ws.is_cuda:
            # torch's CPU convolutions round a batch of one differently from a batch of several (the heads' grouped convolutions, ~4e-6 of the range): the
            # promise that frozen frames do not depend on views_per_step is kept by evaluating CPU views singly — where there is no launch to amortise
            step = 1
        for f0 in range(0, n_frames, step):
            c = cameras[f0:f0 + step]
            b = c.shape[0]
            with _frozen_draws(frozen[0].expand(b, -1, -1, -1), frozen[1].repeat(b, 1)) if frozen is not None else contextlib.nullcontext():
                if per_frame:
                    out = G.synthesis(ws[f0:f0 + b], c, neural_rendering_resolution=nrr, **synthesis_kwargs)
                else:
                    G._last_planes = planes                                # (the slot is the argument of this internal call; restored below)
                    out = G.synthesis(ws, c, neural_rendering_resolution=nrr, use_cached_backbone=True, **synthesis_kwargs)
            if dst is None:
                dst = _alloc_frames(out, n_frames, depth_range, label_mode)
                pal = _palette_for(out, palette)
                if pal is not None and ws.is_cuda:
                    pal = pal.to(ws.device)                                # one copy per video, read in place by every launch
            frame_finish(_frame_jobs(out, {k: v[f0:f0 + b] for k, v in dst.items()}, pal, depth_range))
            if return_float:
                for k, v in out.items():
                    if torch.is_tensor(v):
                        floats.setdefault(k, []).append(v)
    finally:
        G._last_planes = found
    if return_float:
        dst['float'] = {k: torch.cat(v) for k, v in floats.items()}
    return dst


# ---- the scripts ------------------------------------------------------------------------------------------------------------
def _check_resample(who, size, resample):
    """The ``size=`` / ``resample=`` pair of the scripts, checked before anything is rendered."""
    if resample not in rs.FILTERS:
        raise ValueError(f'{who}: resample must be one of {rs.FILTERS}, got {resample!r}')
    if size is not None:
        rs._check_size(size, who)


def resize_clips(frames, size, resample='lanczos'):
    """The uint8 clips of a frames dict at ``size`` ((width, height) or an int), where they are (``resample.resize``): 'image' through the filter
    ``resample``; 'label' and 'label_index' ALWAYS through 'nearest' — a label is never blended; anything else in the dict ('depth', 'float') keeps its size.
    ``size=None``: the dict as it is."""
    if size is None:
        return frames
    for key, how in (('image', resample), ('label', 'nearest'), ('label_index', 'nearest')):
        if key in frames:
            frames[key] = rs.resize(frames[key], size, how)
    return frames


def image_grid(frames, grid_size, cell=None):
    """Contact sheet: frames [N, H, W, C] or [N, H, W] -> [gh * H, gw * W(, C)] for ``grid_size = (gw, gh)``, row-major (training_loop.py:74-89).
    ``cell`` ((width, height) or an int): every frame is resized to it first (``resample.thumbnails``: Lanczos, on the frames' device) — a thumbnail sheet."""
    gw, gh = grid_size
    if cell is not None:
        frames = rs.thumbnails(frames, cell)
    n, h, w = frames.shape[:3]
    if gw * gh != n:
        raise ValueError(f'image_grid: {n} frames do not fill a {gw} x {gh} grid')
    t = frames.reshape(gh, gw, h, w, -1).permute(0, 2, 1, 3, 4).reshape(gh * h, gw * w, -1)
    return t if frames.ndim == 4 else t[..., 0]


@torch.no_grad()
def generate_video(G, ws, cfg='seg2cat', path=None, path_label=None, n_frames=120, fps=60, gif='pil', format='gif', psnr=None, ssim=None, size=None,
                   resample='lanczos', ms_ssim=None, **render_kwargs):
    """generate_video.py after its inputs: the ``cfg`` cameras (``video_cameras``) at the script's ray resolution with ``noise_mode='const'``, rendered by
    ``render_views`` (its keyword arguments pass through); ``path`` / ``path_label`` receive the two GIFs the script writes with imageio at 60 fps.
    ``gif='pil'``: through ``mesh.save_gif``, PIL quantising every frame on the host.  ``gif='device'``: the image through ``video.save_gif`` (one palette for
    the clip, made and applied where the frames are) and the label video losslessly through ``video.save_gif_indexed`` — ``label_index`` with the frames'
    palette, or the edge generators' grey frames with a grey ramp.  ``format='avi'``: both clips in true colour as Motion-JPEG AVIs through
    ``video.save_avi``, encoded where the frames are (``gif`` plays no part).  ``format='apng'``: both clips losslessly as animated PNGs through
    ``video.save_apng``, encoded where the frames are — the image as RGB, the label video as palette indices (``label_index`` with the frames' palette) or,
    for the edge generators, as 8-bit grey.  ``psnr`` / ``ssim`` / ``ms_ssim`` (``format='avi'`` only, one of them): a target for the image clip instead of the default
    quality — ``video.jpeg_quality_for`` picks the setting where the frames are, the dict gains 'jpeg_quality': ``(quality, metrics, met)``, and the label
    clip goes through ``video.save_avi`` with the same target.  ``size`` ((width, height) or an int): the clips are resized where they are before the
    writer and before any quality search (``resize_clips``: the image through the filter ``resample``, label and index frames through 'nearest'), and the
    dict holds them at that size; ``size=None`` writes the same bytes as ever.  Returns ``render_views``' dict."""
    from .video.clip import check_clip_options, save_clip
    check_clip_options('generate_video', gif, format, psnr, ssim, ms_ssim)
    _check_resample('generate_video', size, resample)
    cams = video_cameras(G, cfg, n_frames).to(ws.device)
    render_kwargs.setdefault('noise_mode', 'const')
    render_kwargs.setdefault('neural_rendering_resolution', VIDEO_CFG[cfg]['neural_rendering_resolution'])
    frames = resize_clips(render_views(G, ws, cams, **render_kwargs), size, resample)
    how = dict(fps=fps, format=format, gif=gif, psnr=psnr, ssim=ssim, ms_ssim=ms_ssim, who='generate_video')
    if path is not None:
        chosen = save_clip(path, frames['image'], **how)
        if chosen is not None:
            frames['jpeg_quality'] = chosen
    if path_label is not None:
        if 'label' not in frames:
            raise ValueError(f'generate_video: {type(G).__name__} has no label output for path_label')
        indices, pal = frames.get('label_index'), render_kwargs.get('palette')  # (the edge generators' frames are grey, [F, H, W], and have no indices)
        if indices is not None:                                                # default_palette(c) is the first c rows of default_palette(256)
            pal = mesh.default_palette(256) if pal is None else torch.as_tensor(pal)
        save_clip(path_label, frames['label'], indices=indices, palette=pal, **how)
    return frames


@torch.no_grad()
def generate_sample(G, ws, camera, path_color=None, path_label=None, palette=None, png='pil', **synthesis_kwargs):
    """generate_samples.py:108-120 after its inputs: one ``G.synthesis(ws, camera, noise_mode='const')`` finished by ``finish_frames``; the image and the
    label map go to ``path_color`` / ``path_label`` through PIL.  ``png='device'``: through ``video.save_png`` instead, encoded where the frames are — the
    image as RGB, the label map as palette indices where ``label_index`` exists (the same pixels, a smaller file).  ``camera`` is a [25] or [N, 25] label.
    ``size=None, resample='lanczos'`` (keywords, taken out of ``synthesis_kwargs``: the positional parameters stay as they were): as for ``generate_video``
    (``resize_clips`` before the files are written).  Returns ``finish_frames``' dict."""
    from PIL import Image
    if png not in ('pil', 'device'):
        raise ValueError(f"generate_sample: png must be 'pil' or 'device', got {png!r}")
    size, resample = synthesis_kwargs.pop('size', None), synthesis_kwargs.pop('resample', 'lanczos')
    _check_resample('generate_sample', size, resample)
    camera = torch.as_tensor(camera, dtype=torch.float32).to(ws.device).reshape(-1, 25)
    synthesis_kwargs.setdefault('noise_mode', 'const')
    out = G.synthesis(ws, camera, **synthesis_kwargs)
    frames = resize_clips(finish_frames(out, palette=palette, label_mode='grey' if getattr(G, 'data_type', None) == 'edge' else 'auto'), size, resample)
    for p, key in ((path_color, 'image'), (path_label, 'label')):
        if p is not None and png == 'device':
            from . import video
            if key == 'label' and 'label_index' in frames:
                video.save_png(p, frames['label_index'][0], mode='P', palette=mesh.default_palette(256) if palette is None else torch.as_tensor(palette))
            else:
                video.save_png(p, frames[key][0])
        elif p is not None:
            Image.fromarray(frames[key][0].cpu().numpy()).save(p)
    return frames
