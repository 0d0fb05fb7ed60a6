"""Surface casting: geometry frames straight from the density field, without a lattice and without a mesh.

The offline way to see a generator's shape is applications/extract_mesh.py:60-99 — a 512^3 density lattice (``shape.sigma_grid``),
marching cubes (``shape.marching_cubes``), then the rasterizer (``mesh.render``): 134 M decoder evaluations before the first pixel.  A
view needs the density only along the camera's rays, and only up to the first crossing of the level set:

    frames = surface.render(G, ws, views.video_cameras(G, 'seg2cat', 8), resolution=512)              # uint8 [8, 512, 512, 3]
    hit = surface.cast(G, ws, cameras, resolution=512)                                              # SurfaceHit [V, R, R(, 3)]
    frames = surface.shade(hit, cameras[:, :16], mode='normal')

* ``cast_rays``: the definition — march, bisection, central differences — over any callable density.
* ``cast``: the same for a generator's cameras; device tensors run the backbone once and ONE ``p3d_surface_cast`` launch over the one
  plane set (csrc/surface.hip), CPU tensors and other generators ``cast_rays`` over ``G.sample_mixed``.
* ``shade``: frames from a ``SurfaceHit`` — ``mesh.shade``'s headlight rule with the density gradient for a normal, or a normal map.
* ``render`` / ``geometry_video``: the two together, with grey, normal, decoder-colour or label albedo; a turntable of them.

Device tensors run csrc/surface.hip, CPU tensors the formulation below, written operation by operation: it is the definition
(include/p3d_hip.h, "surface casting").  The cast kernel equals ``cast_rays`` over the point kernel (``renderer.fused_sample_points``)
bit for bit, the shade kernel's bytes equal ``_shade_cpu``'s.
"""
import ctypes
from typing import NamedTuple

import torch

from . import _lib, mesh, shape, texture, views
from ._lib import _f32, _i32, _vp
from .training.volumetric_rendering import renderer as _rmod

GREY = mesh.GREY
MIN_STEPS, MAX_STEPS, MAX_REFINE = 2, 4096, 24          # p3d_surface_cast's limits
_MODES = {'lambert': 0, 'normal': 1}
_RAY_BYTES = 1024                                        # what one ray of a chunk is budgeted at: its points, the features and hidden units behind them

# (renderer.fused_surface_cast, which makes the cast's call, declares the same signature)
_lib.register('p3d_surface_cast', ctypes.c_int, [_vp, _vp, ctypes.POINTER(_rmod._RenderDesc), _vp, _vp, _f32, _f32, _i32, _i32, _f32, _f32, _f32, _i32] + [_vp] * 5)
_lib.register('p3d_surface_shade', ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _i32, _i32, _i32, _i32, _vp, _vp])      # csrc/surface.hip


class SurfaceHit(NamedTuple):
    """Per ray: ``hit`` uint8 (1 where the ray crosses the level set), ``depth`` float32 (+inf on a miss), ``position`` float32 [..., 3]
    (o + depth d; zero on a miss), ``grad`` float32 [..., 3] (the unnormalised central density differences there, pointing INTO the
    shape; zero on a miss, and not finite at every hit)."""
    hit: torch.Tensor
    depth: torch.Tensor
    position: torch.Tensor
    grad: torch.Tensor


# ---- the definition -----------------------------------------------------------------------------------------------------------
def _check_cast(steps, refine):
    if not MIN_STEPS <= int(steps) <= MAX_STEPS:
        raise ValueError(f'surface cast: steps must be {MIN_STEPS} .. {MAX_STEPS}, got {steps}')
    if not 0 <= int(refine) <= MAX_REFINE:
        raise ValueError(f'surface cast: refine must be 0 .. {MAX_REFINE}, got {refine}')


def _outside(p, half_box):
    """Box clip: any |component| > half_box (a NaN component is not outside); ``half_box <= 0`` clips nothing."""
    if half_box <= 0:
        return torch.zeros(p.shape[:-1], dtype=torch.bool, device=p.device)
    return (p.abs() > half_box).any(dim=-1)


def _cast_chunk(sigma_fn, o, d, near, dt, steps, refine, thr, eps, half_box):
    """``cast_rays`` for one chunk of rays; near, dt, thr, eps are 0-dim float32 tensors on the rays' device, half_box a float32 value.  Every ray's point is
    evaluated at every step (a finished ray's result is ignored, as the kernel's): no value depends on which rays share a call."""
    r, dev = o.shape[0], o.device
    searching = torch.ones([r], dtype=torch.bool, device=dev)
    found, bisect = torch.zeros_like(searching), torch.zeros_like(searching)
    lo, hi = near.expand(r).clone(), near.expand(r).clone()
    for i in range(steps):
        if not bool(searching.any()):
            break
        ti = near + torch.tensor(float(i), dtype=torch.float32, device=dev) * dt
        p = o + ti * d
        above = searching & ~_outside(p, half_box) & (sigma_fn(p) > thr)              # (NaN > thr is False)
        lo = torch.where(searching & ~above, ti, lo)
        hi = torch.where(above, ti, hi)
        found |= above
        if i > 0:
            bisect |= above
        searching &= ~above
    if bool(bisect.any()):
        for _ in range(refine):
            tm = 0.5 * (lo + hi)
            p = o + tm[:, None] * d
            above = bisect & ~_outside(p, half_box) & (sigma_fn(p) > thr)
            hi = torch.where(above, tm, hi)
            lo = torch.where(bisect & ~above, tm, lo)
    depth = torch.where(found, hi, torch.full_like(hi, float('inf')))
    position = torch.where(found[:, None], o + hi[:, None] * d, torch.zeros_like(o))
    grad = torch.zeros_like(o)
    if bool(found.any()):
        for a in range(3):
            plus, minus = position.clone(), position.clone()
            plus[:, a] = position[:, a] + eps
            minus[:, a] = position[:, a] - eps
            grad[:, a] = torch.where(found, sigma_fn(plus) - sigma_fn(minus), torch.zeros_like(hi))
    return found.to(torch.uint8), depth, position, grad


@torch.no_grad()
def cast_rays(sigma_fn, ray_o, ray_d, near, far, steps=128, refine=8, threshold=50.0, eps=None, half_box=None, max_bytes=1 << 30):
    """The surface cast of rays ``ray_o``, ``ray_d`` [P, 3] through the density ``sigma_fn(points [Q, 3]) -> [Q]``, in float32 on the rays'
    device, every operation a rounded one:

    samples   t_i = near + float(i) * dt for i = 0 .. steps - 1, dt = float32((far - near) / (steps - 1)); p(t) = o + t * d;
    box clip  ``half_box`` > 0: a point with any |component| > half_box is outside — never above the threshold, its density unused;
    hit       the first i with sigma(p(t_i)) > threshold.  i = 0: depth = t_0.  Else lo = t_{i-1}, hi = t_i and ``refine`` times
              tm = 0.5 * (lo + hi); sigma(p(tm)) > threshold ? hi = tm : lo = tm; then depth = hi;
    gradient  position = o + depth * d; grad[a] = sigma(position + eps e_a) - sigma(position - eps e_a) (no box clip, unnormalised;
              not finite where the density or the position is not);
    miss      hit 0, depth +inf, position and grad zero.  A NaN density is never a hit.

    ``eps`` defaults to 1 / 256.  Rays go through in chunks that keep the evaluation of one step under ``max_bytes``.  Returns a
    ``SurfaceHit`` of [P] / [P, 3] tensors."""
    _check_cast(steps, refine)
    o = ray_o.detach().to(torch.float32).reshape(-1, 3)
    d = ray_d.detach().to(device=o.device, dtype=torch.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError(f'cast_rays: {o.shape[0]} origins for {d.shape[0]} directions')
    scalar = lambda v: torch.tensor(float(v), dtype=torch.float32, device=o.device)
    steps, refine = int(steps), int(refine)
    args = (scalar(near), scalar((float(far) - float(near)) / (steps - 1)), steps, refine, scalar(threshold), scalar(1 / 256 if eps is None else eps),
            float(scalar(0.0 if half_box is None else half_box)))
    chunk = max(1, int(max_bytes) // _RAY_BYTES)
    parts = [_cast_chunk(sigma_fn, o[s:s + chunk], d[s:s + chunk], *args) for s in range(0, o.shape[0], chunk)]
    if not parts:
        return SurfaceHit(torch.zeros([0], dtype=torch.uint8, device=o.device), torch.zeros([0], device=o.device), torch.zeros([0, 3], device=o.device),
                          torch.zeros([0, 3], device=o.device))
    return SurfaceHit(*(torch.cat(t) for t in zip(*parts)))


# ---- a generator's cameras ------------------------------------------------------------------------------------------------------
def _ray_range(G, near, far):
    rk = G.rendering_kwargs
    near, far = rk.get('ray_start') if near is None else near, rk.get('ray_end') if far is None else far
    if isinstance(near, str) or isinstance(far, str) or near is None or far is None:
        raise ValueError(f"surface cast: the generator's ray range is ({near!r}, {far!r}); pass near= and far= as numbers")
    return float(near), float(far)


def _planes5(planes):
    return planes if planes.ndim == 5 else planes.view(len(planes), 3, 32, planes.shape[-2], planes.shape[-1])


@torch.no_grad()
def cast(G, ws, cameras, resolution=512, near=None, far=None, steps=128, refine=8, threshold=50.0, eps=None, clip_box=True, planes=None,
         max_bytes=1 << 30, **synthesis_kwargs):
    """The surface {sigma > threshold} of the latent ``ws`` [1, num_ws, w_dim] as the cameras ``cameras`` [V, 25] see it, resolution^2 rays
    each from G's ``RaySampler``: a ``SurfaceHit`` shaped [V, R, R(, 3)] on ws's device.

    ``near`` / ``far`` default to ``rendering_kwargs['ray_start' / 'ray_end']`` (ValueError when those are 'auto' and no numbers are
    given), ``eps`` to box_warp / 256, ``noise_mode`` to 'const'; ``clip_box`` keeps the surface inside [-box_warp / 2, box_warp / 2]^3
    (beyond it the planes are zero-padded and the decoder's answer is not the shape's).  ``planes``: the backbone's output for ``ws`` when
    the caller holds it (``EditSession``); no backbone pass is made then.

    Device tensors of a generator ``shape.sigma_grid`` has a lattice kernel for run the backbone once and one ``p3d_surface_cast`` launch:
    V ray sets over the one plane set.  CPU tensors and other generators run ``cast_rays`` over ``G.sample_mixed`` (on a device, under
    ``renderer.fused_policy``: a warning, or an error under 'require')."""
    if ws.ndim != 3 or ws.shape[0] != 1:
        raise ValueError(f'surface.cast: one latent at a time, ws [1, num_ws, w_dim] (got {tuple(ws.shape)})')
    cameras = torch.as_tensor(cameras, dtype=torch.float32).to(ws.device)
    if cameras.ndim != 2 or cameras.shape[1] != 25:
        raise ValueError(f'surface.cast: cameras must be [V, 25], got {tuple(cameras.shape)}')
    _check_cast(steps, refine)
    near, far = _ray_range(G, near, far)
    box = float(G.rendering_kwargs['box_warp'])
    eps = box / 256 if eps is None else float(eps)
    half_box = box * 0.5 if clip_box else 0.0
    synthesis_kwargs.setdefault('noise_mode', 'const')
    v, r = cameras.shape[0], int(resolution)
    ray_o, ray_d = G.ray_sampler(cameras[:, :16].view(-1, 4, 4), cameras[:, 16:25].view(-1, 3, 3), r)
    reason = shape._lattice_reason(G, ws)
    if reason is None:
        planes = _planes5(shape._planes(G, ws, **synthesis_kwargs) if planes is None else planes)
        out = _rmod.fused_surface_cast(planes, G.decoder, ray_o, ray_d, G.rendering_kwargs, near, far, steps, refine, threshold, eps, half_box,
                                       raster_width=r if r % 8 == 0 else 0)
    else:
        _rmod._tensor_op_guard('surface.cast', ws.is_cuda, reason, required='surface cast kernel required but unavailable',
                               instead='cast_rays over G.sample_mixed, not the surface cast kernel')
        if planes is None:
            sigma_fn = lambda pts: G.sample_mixed(pts[None], None, ws=ws, **synthesis_kwargs)['sigma'].reshape(-1)
        else:
            sigma_fn = lambda pts: G.renderer.run_model(_planes5(planes), G.decoder, pts[None], None, G.rendering_kwargs)['sigma'].reshape(-1)
        out = cast_rays(sigma_fn, ray_o.reshape(-1, 3), ray_d.reshape(-1, 3), near, far, steps, refine, threshold, eps, half_box, max_bytes)
    hit, depth, position, grad = out
    return SurfaceHit(hit.reshape(v, r, r), depth.reshape(v, r, r), position.reshape(v, r, r, 3), grad.reshape(v, r, r, 3))


# ---- shading ----------------------------------------------------------------------------------------------------------------
def _shade_cpu(hit, grad, albedo, cams, ambient, mode, background):
    """The definition of ``shade`` in float64, one torch operation per rounding: hit [V, H, W], grad [V, H, W, 3], albedo uint8
    [V, H, W, 3] or None, cams float32 [V, 16]."""
    g = grad.double()
    g = torch.where(torch.isfinite(g).all(dim=-1, keepdim=True), g, torch.zeros_like(g))      # a non-finite gradient counts as the zero gradient
    g0, g1, g2 = g.unbind(-1)
    nn = g0 * g0
    nn = nn + g1 * g1
    nn = nn + g2 * g2
    if mode == 'normal':
        n = nn.sqrt()
        ok = n > 0
        u = torch.where(ok[..., None], -g / torch.where(ok, n, torch.ones_like(n))[..., None], torch.zeros_like(g))
        out = torch.floor((u * 0.5 + 0.5) * 255.0 + 0.5).clamp(0, 255).to(torch.uint8)
    else:
        f0, f1, f2 = (cams[:, j].double()[:, None, None] for j in (2, 6, 10))
        ff = f0 * f0
        ff = ff + f1 * f1
        ff = ff + f2 * f2
        dot = g0 * f0
        dot = dot + g1 * f1
        dot = dot + g2 * f2
        den = nn.sqrt() * ff.sqrt()
        ok = den > 0
        cosv = torch.where(ok, dot.abs() / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(den))
        amb = float(torch.tensor(ambient, dtype=torch.float32))
        shade_ = amb + (1.0 - amb) * cosv
        alb = torch.full_like(g, float(GREY)) if albedo is None else albedo.double()
        out = torch.floor(alb * shade_[..., None] + 0.5).clamp(0, 255).to(torch.uint8)
    return torch.where(hit[..., None] != 0, out, torch.tensor(background, dtype=torch.uint8).expand_as(out))


def shade(hit, cam2world, albedo=None, mode='lambert', background=(255, 255, 255), ambient=0.3):
    """uint8 [V, H, W, 3] frames from a ``SurfaceHit`` shaped [V, H, W(, 3)] and the cameras' cam2world [V, 4, 4] (or [V, 16], or the
    [V, 25] camera labels).  With g the density gradient and f the camera's forward axis (entries 2, 6, 10 of cam2world), in float64:

    'lambert'  cos = |g . f| / (|g| |f|), 0 where the denominator is 0; shade = ambient + (1 - ambient) cos; byte = floor(albedo * shade
               + 0.5) clamped — ``mesh.shade``'s rule; ``albedo`` uint8 [V, H, W, 3], or None for ``mesh.GREY``;
    'normal'   byte = floor((-g / |g| * 0.5 + 0.5) * 255 + 0.5) per component, 128 where |g| is 0.

    A gradient with a non-finite component counts as the zero gradient; ``background`` where ``hit.hit`` is 0.  Device tensors run
    ``p3d_surface_shade``, CPU tensors the definition: the same bytes."""
    if mode not in _MODES:
        raise ValueError(f"surface.shade: mode must be 'lambert' or 'normal', got {mode!r}")
    h, g = hit.hit, hit.grad
    if h.ndim != 3 or tuple(g.shape) != tuple(h.shape) + (3,):
        raise ValueError(f'surface.shade: hit must be [V, H, W] and grad [V, H, W, 3], got {tuple(h.shape)} and {tuple(g.shape)}')
    n, height, width = h.shape
    dev = h.device
    h = h.detach().to(torch.uint8).contiguous()
    g = g.detach().to(device=dev, dtype=torch.float32).contiguous()
    cams = torch.as_tensor(cam2world, dtype=torch.float32).detach()
    cams = cams.reshape(n, -1) if n else cams.reshape(0, 16)
    if cams.shape[1] not in (16, 25):
        raise ValueError(f'surface.shade: cam2world {tuple(torch.as_tensor(cam2world).shape)} is not [{n}, 4, 4], [{n}, 16] or [{n}, 25]')
    cams = cams[:, :16]
    cams = cams.to(dev).contiguous()
    if albedo is not None:
        albedo = torch.as_tensor(albedo).detach().to(device=dev, dtype=torch.uint8).contiguous()
        if tuple(albedo.shape) != (n, height, width, 3):
            raise ValueError(f'surface.shade: albedo must be uint8 [{n}, {height}, {width}, 3], got {tuple(albedo.shape)}')
    bg = tuple(int(v) & 255 for v in background)
    if not h.is_cuda:
        return _shade_cpu(h, g, albedo, cams, ambient, mode, bg)
    rgb = torch.empty([n, height, width, 3], dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().p3d_surface_shade(_lib.ptr(h), _lib.ptr(g), _lib.ptr(albedo), _lib.ptr(cams), n, height, width, float(ambient), _MODES[mode], *bg,
                                            _lib.ptr(rgb), _lib.stream_of(rgb)), 'surface_shade')
    return rgb


# ---- frames -------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def render(G, ws, cameras, resolution=512, color='grey', palette=None, background=(255, 255, 255), ambient=0.3, return_hit=False, **cast_kwargs):
    """Geometry frames uint8 [V, R, R, 3] of the latent ``ws`` [1, num_ws, w_dim] at ``cameras`` [V, 25]: ``cast`` then ``shade``.

    color  'grey': uniform ``mesh.GREY`` under the headlight; 'normal': the normal map; 'rgb': the decoder's own colour at the hit
           positions (``texture.vertex_rgb``) under the headlight; 'label': the label colour there (``mesh.vertex_labels`` with
           ``palette``).  'rgb' and 'label' query ``G.sample_mixed`` at the hit positions, which runs the backbone once more.
    ``cast_kwargs`` go to ``cast``.  With ``return_hit`` also the ``SurfaceHit``."""
    if color not in ('grey', 'normal', 'rgb', 'label'):
        raise ValueError(f"surface.render: color must be 'grey', 'normal', 'rgb' or 'label', got {color!r}")
    cameras = torch.as_tensor(cameras, dtype=torch.float32).to(ws.device)
    hit = cast(G, ws, cameras, resolution, **cast_kwargs)
    albedo = None
    if color in ('rgb', 'label'):
        pts = hit.position.reshape(-1, 3)
        colors = texture.vertex_rgb(G, ws, pts) if color == 'rgb' else mesh.vertex_labels(G, ws, pts, palette)[1]
        albedo = colors.reshape(hit.position.shape)
    frames = shade(hit, cameras[:, :16], albedo, 'normal' if color == 'normal' else 'lambert', background, ambient)
    return (frames, hit) if return_hit else frames


@torch.no_grad()
def geometry_video(G, ws, cfg='seg2cat', n_frames=120, views_per_step=4, resolution=512, color='grey', path=None, fps=60, **render_kwargs):
    """The geometry turntable of ``ws`` [1, num_ws, w_dim]: ``render`` over ``views.video_cameras(G, cfg, n_frames)``, ``views_per_step``
    cameras per cast launch, the backbone run once for all of them where the cast kernel serves.  uint8 [n_frames, R, R, 3] on ws's
    device; with ``path`` also written as a GIF (``mesh.save_gif``)."""
    step = int(views_per_step)
    if step < 1:
        raise ValueError(f'geometry_video: views_per_step must be >= 1, got {views_per_step}')
    cameras = views.video_cameras(G, cfg, n_frames).to(ws.device)
    kw = dict(render_kwargs)
    if kw.get('planes') is None and shape._lattice_reason(G, ws) is None:
        kw['planes'] = shape._planes(G, ws, noise_mode=kw.get('noise_mode', 'const'))
    frames = [render(G, ws, cameras[s:s + step], resolution, color=color, **kw) for s in range(0, cameras.shape[0], step)]
    out = torch.cat(frames) if frames else torch.empty([0, int(resolution), int(resolution), 3], dtype=torch.uint8, device=ws.device)
    if path is not None:
        mesh.save_gif(path, out.cpu().numpy(), fps=fps)
    return out
