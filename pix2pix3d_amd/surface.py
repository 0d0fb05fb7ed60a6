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
* ``occlusion_rays``: the definition of the second ray stage — per surface point, how many of a set of directions it faces and how many
  of those short rays reach their end unblocked; ``occlusion``: the same for a ``SurfaceHit`` of a generator, ONE
  ``p3d_surface_occlusion`` launch for all views; ``sphere_directions`` / ``light_directions``: the direction sets of ambient occlusion
  and of (soft) shadows; ``shade_lit``: the shade with a directional light and those counts (``render(ao=..., shadows=..., light=...)``).

Device tensors run csrc/surface.hip, CPU tensors the formulation below, written operation by operation: it is the definition
(include/p3d_hip.h, "surface casting").  The cast kernel equals ``cast_rays`` over the point kernel (``renderer.fused_sample_points``)
bit for bit, the shade kernel's bytes equal ``_shade_cpu``'s; the occlusion kernel's counts equal ``occlusion_rays``' over the point kernel, the lit
shade's bytes ``_shade_lit_cpu``'s.
"""
import math
from typing import NamedTuple

import torch

from . import _lib, mesh, shape, texture, views
from .resample import resize
from .training.volumetric_rendering import renderer as _rmod

GREY = mesh.GREY
MIN_STEPS, MAX_STEPS, MAX_REFINE = 2, 4096, 24          # p3d_surface_cast's limits
MAX_DIRECTIONS = 255                                     # p3d_surface_occlusion's limit (its counts are bytes); its steps are 1 .. MAX_STEPS
_MODES = {'lambert': 0, 'normal': 1}
_RAY_BYTES = 1024                                        # what one ray of a chunk is budgeted at: its points, the features and hidden units behind them


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


# ---- the second ray stage: the definition ---------------------------------------------------------------------------------------
def _check_occlusion(n_directions, steps):
    if not 1 <= int(n_directions) <= MAX_DIRECTIONS:
        raise ValueError(f'surface occlusion: 1 .. {MAX_DIRECTIONS} directions, got {n_directions}')
    if not 1 <= int(steps) <= MAX_STEPS:
        raise ValueError(f'surface occlusion: steps must be 1 .. {MAX_STEPS}, got {steps}')


def _occlusion_chunk(sigma_fn, o, f, active, dirs, ds, steps, thr, half_box):
    """``occlusion_rays`` for one chunk of points; ds, thr are 0-dim float32 tensors on the points' device.  Every point's sample is evaluated at every
    step of every direction some point of the chunk still needs (a finished or unused ray's result is ignored, as the kernel's): no value depends on
    which points share a call."""
    p_, dev = o.shape[0], o.device
    total, open_ = torch.zeros([p_], dtype=torch.uint8, device=dev), torch.zeros([p_], dtype=torch.uint8, device=dev)
    on = active != 0
    for k in range(dirs.shape[0]):
        d = dirs[k]
        dot = f[:, 0] * d[0]
        dot = dot + f[:, 1] * d[1]
        dot = dot + f[:, 2] * d[2]
        used = on & (dot > 0)                                                         # (NaN > 0 is False)
        blocked = torch.zeros_like(used)
        for j in range(steps):
            going = used & ~blocked
            if not bool(going.any()):
                break
            sj = torch.tensor(float(j + 1), dtype=torch.float32, device=dev) * ds
            p = o + sj * d
            blocked |= going & ~_outside(p, half_box) & (sigma_fn(p) > thr)           # (NaN > thr is False)
        total += used.to(torch.uint8)
        open_ += (used & ~blocked).to(torch.uint8)
    return open_, total


@torch.no_grad()
def occlusion_rays(sigma_fn, origin, facing, active, directions, reach, steps, threshold, half_box=None, max_bytes=1 << 30):
    """What short rays from surface points find: for the points ``origin`` [P, 3] whose surface faces ``facing`` [P, 3] (``active`` uint8 [P]: 0 switches
    a point off), rays along each of ``directions`` [K, 3] through the density ``sigma_fn(points [Q, 3]) -> [Q]``, in float32 on the points' device,
    every operation a rounded one:

    samples   s_j = float(j + 1) * ds for j = 0 .. steps - 1, ds = float32(reach / steps); the point is o + s_j * d per component;
    used      direction k is used by point p iff active[p] != 0 and ((f_x d_x) + (f_y d_y)) + (f_z d_z) > 0 (a NaN: not used);
    blocked   a used direction is blocked iff some sample lies inside the box (``cast_rays``' clip: ``half_box`` > 0 and any |component| >
              half_box is outside) and has sigma > threshold.  A NaN density never blocks.

    Returns ``(open, total)``, uint8 [P]: the number of used directions that are not blocked, and the number of used directions; both 0 for
    an inactive point.  1 <= K <= 255, 1 <= steps <= 4096.  Points go through in chunks that keep one evaluation under ``max_bytes``."""
    o = origin.detach().to(torch.float32).reshape(-1, 3)
    dev = o.device
    f = facing.detach().to(device=dev, dtype=torch.float32).reshape(-1, 3)
    act = torch.as_tensor(active).detach().to(device=dev).reshape(-1)
    dirs = torch.as_tensor(directions).detach().to(device=dev, dtype=torch.float32)
    if dirs.ndim != 2 or dirs.shape[1] != 3:
        raise ValueError(f'occlusion_rays: directions must be [K, 3], got {tuple(dirs.shape)}')
    if f.shape != o.shape or act.shape[0] != o.shape[0]:
        raise ValueError(f'occlusion_rays: {o.shape[0]} origins for {f.shape[0]} facings and {act.shape[0]} flags')
    _check_occlusion(dirs.shape[0], steps)
    scalar = lambda v: torch.tensor(float(v), dtype=torch.float32, device=dev)
    steps = int(steps)
    args = (dirs, scalar(float(reach) / steps), steps, scalar(threshold), float(scalar(0.0 if half_box is None else half_box)))
    chunk = max(1, int(max_bytes) // _RAY_BYTES)
    parts = [_occlusion_chunk(sigma_fn, o[s:s + chunk], f[s:s + chunk], act[s:s + chunk], *args) for s in range(0, o.shape[0], chunk)]
    if not parts:
        return torch.zeros([0], dtype=torch.uint8, device=dev), torch.zeros([0], dtype=torch.uint8, device=dev)
    return tuple(torch.cat(t) for t in zip(*parts))


def sphere_directions(k):
    """``k`` unit vectors spread over the whole sphere, float32 [k, 3]: the spherical Fibonacci set z_i = 1 - (2 i + 1) / k, azimuth i pi (3 - sqrt 5),
    computed in float64 on the host and rounded once.  Deterministic; about half of them face any one surface point."""
    k = int(k)
    if k < 1:
        raise ValueError(f'sphere_directions: k must be >= 1, got {k}')
    i = torch.arange(k, dtype=torch.float64)
    z = 1.0 - (2.0 * i + 1.0) / k
    r = torch.sqrt((1.0 - z * z).clamp_min(0.0))
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    v = torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], dim=-1)
    return (v / v.norm(dim=-1, keepdim=True)).to(torch.float32)


def light_directions(light, samples=1, spread=0.0):
    """The rays towards a light, float32 [V, K, 3] on the host, from ``light`` [3] or [V, 3] (the direction TOWARDS it).  ``samples`` = 1: the light
    itself, as given (a ray's reach scales with its length: pass a unit vector).  Else K = ``samples`` unit vectors in the cone of half-angle
    ``spread`` (radians) about it — a light of that angular size, for soft shadows: cos(theta_i) = 1 - (i + 0.5) / K * (1 - cos spread), azimuth
    i pi (3 - sqrt 5) about the light, in float64 and rounded once.  Deterministic."""
    l32 = torch.as_tensor(light, dtype=torch.float32).detach().cpu()
    if l32.ndim == 1:
        l32 = l32[None]
    if l32.ndim != 2 or l32.shape[1] != 3:
        raise ValueError(f'light_directions: light must be [3] or [V, 3], got {tuple(l32.shape)}')
    k = int(samples)
    if k < 1:
        raise ValueError(f'light_directions: samples must be >= 1, got {samples}')
    if k == 1:
        return l32[:, None, :].clone()
    a = l32.double()
    a = a / a.norm(dim=-1, keepdim=True)
    helper = torch.nn.functional.one_hot(a.abs().argmin(dim=-1), 3).double()           # the axis the light is furthest from
    t = torch.linalg.cross(helper, a)
    t = t / t.norm(dim=-1, keepdim=True)
    b = torch.linalg.cross(a, t)
    i = torch.arange(k, dtype=torch.float64)
    cos_t = 1.0 - (i + 0.5) / k * (1.0 - math.cos(float(spread)))
    sin_t = torch.sqrt((1.0 - cos_t * cos_t).clamp_min(0.0))
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    v = (sin_t * torch.cos(phi))[None, :, None] * t[:, None, :] + (sin_t * torch.sin(phi))[None, :, None] * b[:, None, :] + cos_t[None, :, None] * a[:, None, :]
    return (v / v.norm(dim=-1, keepdim=True)).to(torch.float32)


def world_light(light, cam2world, space='camera'):
    """The direction towards the light in world space, unit, float32 [V, 3] on the host: ``light`` is a 3-vector in 'world' space, or in 'camera' space
    (x right, y down, z forward: it moves with the camera) and is then rotated by the 3 x 3 block of every ``cam2world`` [V, 16 | 25 | 4, 4]; float64,
    rounded once."""
    if space not in ('camera', 'world'):
        raise ValueError(f"surface: light_space must be 'camera' or 'world', got {space!r}")
    l = torch.as_tensor(light, dtype=torch.float64).detach().cpu().reshape(-1)
    if l.shape[0] != 3 or not float(l.norm()) > 0:
        raise ValueError(f'surface: light must be a non-zero 3-vector, got {tuple(torch.as_tensor(light).shape)}')
    cams = torch.as_tensor(cam2world, dtype=torch.float32).detach().cpu().double()
    cams = cams.reshape(cams.shape[0], -1)[:, :16].reshape(-1, 4, 4)
    w = cams[:, :3, :3] @ l if space == 'camera' else l.expand(cams.shape[0], 3)
    return (w / w.norm(dim=-1, keepdim=True)).to(torch.float32)


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


def occlusion_points(hit, offset):
    """(origin, facing [..., 3] float32, active uint8 [...]) of a ``SurfaceHit``, in float32 torch operations on its device: n = -g / sqrt((g_x g_x +
    g_y g_y) + g_z g_z); active = hit and a finite non-zero |g|; origin = position + offset * n, facing = n; zeros where not active."""
    g = hit.grad.to(torch.float32)
    g0, g1, g2 = g.unbind(-1)
    nn = g0 * g0
    nn = nn + g1 * g1
    nn = nn + g2 * g2
    norm = nn.sqrt()
    active = (hit.hit != 0) & torch.isfinite(norm) & (norm > 0)
    n = torch.where(active[..., None], -g / torch.where(active, norm, torch.ones_like(norm))[..., None], torch.zeros_like(g))
    origin = torch.where(active[..., None], hit.position.to(torch.float32) + torch.tensor(float(offset), dtype=torch.float32, device=g.device) * n,
                         torch.zeros_like(g))
    return origin, n, active.to(torch.uint8)


@torch.no_grad()
def occlusion(G, ws, hit, directions, reach, steps=16, threshold=50.0, offset=None, clip_box=True, planes=None, max_bytes=1 << 30, **synthesis_kwargs):
    """The second ray stage for the ``SurfaceHit`` ``hit`` [V, R, R(, 3)] of ``cast(G, ws, ...)``: from every hit pixel rays of ``steps`` samples up to
    ``reach`` along ``directions`` ([K, 3] for all views, or [V, K, 3]) -> ``(open, total)`` uint8 [V, R, R] as ``occlusion_rays`` defines them, with
    ``occlusion_points(hit, offset)`` for the points: the rays start ``offset`` (default box_warp / 128: two of the gradient's ``eps``, clear of the
    bisection's remaining interval) along the normal off the surface, and only the directions on the normal's side are used.  ``threshold``,
    ``clip_box`` and ``planes`` as for ``cast``: pass the cast's own.

    Routed as ``cast``: device tensors of a generator with a lattice kernel run ONE ``p3d_surface_occlusion`` launch, all V views over the one plane
    set; CPU tensors and other generators ``occlusion_rays`` over ``G.sample_mixed`` (on a device under ``renderer.fused_policy``)."""
    if ws.ndim != 3 or ws.shape[0] != 1:
        raise ValueError(f'surface.occlusion: one latent at a time, ws [1, num_ws, w_dim] (got {tuple(ws.shape)})')
    if hit.hit.ndim != 3 or tuple(hit.grad.shape) != tuple(hit.hit.shape) + (3,) or hit.hit.shape[1] != hit.hit.shape[2]:
        raise ValueError(f'surface.occlusion: hit must be a SurfaceHit of [V, R, R] views, got {tuple(hit.hit.shape)}')
    v, r = hit.hit.shape[0], hit.hit.shape[1]
    dev = hit.hit.device
    dirs = torch.as_tensor(directions, dtype=torch.float32).detach()
    if dirs.ndim == 2:
        dirs = dirs[None].expand(v, -1, -1)
    if dirs.ndim != 3 or dirs.shape[0] != v or dirs.shape[2] != 3:
        raise ValueError(f'surface.occlusion: directions must be [K, 3] or [{v}, K, 3], got {tuple(dirs.shape)}')
    _check_occlusion(dirs.shape[1], steps)
    dirs = dirs.to(dev).contiguous()
    box = float(G.rendering_kwargs['box_warp'])
    half_box = box * 0.5 if clip_box else 0.0
    synthesis_kwargs.setdefault('noise_mode', 'const')
    origin, facing, active = occlusion_points(hit, box / 128 if offset is None else offset)
    origin, facing, active = origin.reshape(v, r * r, 3), facing.reshape(v, r * r, 3), active.reshape(v, r * r)
    reason = shape._lattice_reason(G, ws)
    if reason is None:
        planes = _planes5(shape._planes(G, ws, **synthesis_kwargs) if planes is None else planes)
        open_, total = _rmod.fused_surface_occlusion(planes, G.decoder, origin, facing, active, dirs, G.rendering_kwargs, reach, steps, threshold, half_box,
                                                     raster_width=r if r % 8 == 0 else 0)
    else:
        _rmod._tensor_op_guard('surface.occlusion', ws.is_cuda, reason, required='surface occlusion kernel required but unavailable',
                               instead='occlusion_rays over G.sample_mixed, not the surface occlusion kernel')
        if planes is None:
            sigma_fn = lambda pts: G.sample_mixed(pts[None], None, ws=ws, **synthesis_kwargs)['sigma'].reshape(-1)
        else:
            sigma_fn = lambda pts: G.renderer.run_model(_planes5(planes), G.decoder, pts[None], None, G.rendering_kwargs)['sigma'].reshape(-1)
        parts = [occlusion_rays(sigma_fn, origin[i], facing[i], active[i], dirs[i], reach, steps, threshold, half_box, max_bytes) for i in range(v)]
        open_, total = (torch.stack(t) for t in zip(*parts)) if parts else (torch.zeros([0, r * r], dtype=torch.uint8, device=dev),) * 2
    return open_.reshape(v, r, r), total.reshape(v, r, r)


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


def _shade_operands(who, hit, cam2world, albedo, background):
    """The checked operands of ``shade`` and ``shade_lit``: hit uint8 [V, H, W], grad float32 [V, H, W, 3], cams float32 [V, 16], albedo uint8
    [V, H, W, 3] or None, all contiguous on the hit's device, and the background bytes."""
    h, g = hit.hit, hit.grad
    if h.ndim != 3 or tuple(g.shape) != tuple(h.shape) + (3,):
        raise ValueError(f'{who}: hit must be [V, H, W] and grad [V, H, W, 3], got {tuple(h.shape)} and {tuple(g.shape)}')
    n, height, width = h.shape
    dev = h.device
    h = h.detach().to(torch.uint8).contiguous()
    g = g.detach().to(device=dev, dtype=torch.float32).contiguous()
    cams = torch.as_tensor(cam2world, dtype=torch.float32).detach()
    cams = cams.reshape(n, -1) if n else cams.reshape(0, 16)
    if cams.shape[1] not in (16, 25):
        raise ValueError(f'{who}: cam2world {tuple(torch.as_tensor(cam2world).shape)} is not [{n}, 4, 4], [{n}, 16] or [{n}, 25]')
    cams = cams[:, :16]
    cams = cams.to(dev).contiguous()
    if albedo is not None:
        albedo = torch.as_tensor(albedo).detach().to(device=dev, dtype=torch.uint8).contiguous()
        if tuple(albedo.shape) != (n, height, width, 3):
            raise ValueError(f'{who}: albedo must be uint8 [{n}, {height}, {width}, 3], got {tuple(albedo.shape)}')
    bg = tuple(int(v) & 255 for v in background)
    return h, g, cams, albedo, bg


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
    h, g, cams, albedo, bg = _shade_operands('surface.shade', hit, cam2world, albedo, background)
    n, height, width = h.shape
    if not h.is_cuda:
        return _shade_cpu(h, g, albedo, cams, ambient, mode, bg)
    rgb = torch.empty([n, height, width, 3], dtype=torch.uint8, device=h.device)
    _lib.check(_lib.lib().p3d_surface_shade(_lib.ptr(h), _lib.ptr(g), _lib.ptr(albedo), _lib.ptr(cams), n, height, width, float(ambient), _MODES[mode], *bg,
                                            _lib.ptr(rgb), _lib.stream_of(rgb)), 'surface_shade')
    return rgb


def _shade_lit_cpu(hit, grad, albedo, cams, light, ao, shadow, ambient, background):
    """The definition of ``shade_lit`` in float64, one torch operation per rounding: hit [V, H, W], grad [V, H, W, 3], albedo uint8 [V, H, W, 3] or
    None, cams float32 [V, 16], light float32 [V, 3] or None, ao and shadow (open, total) pairs of uint8 [V, H, W] or None."""
    g = grad.double()
    g = torch.where(torch.isfinite(g).all(dim=-1, keepdim=True), g, torch.zeros_like(g))      # a non-finite gradient counts as the zero gradient
    g0, g1, g2 = g.unbind(-1)
    nn = g0 * g0
    nn = nn + g1 * g1
    nn = nn + g2 * g2
    if light is None:
        l0, l1, l2 = (cams[:, j].double()[:, None, None] for j in (2, 6, 10))                   # the headlight: the camera's forward axis
    else:
        l0, l1, l2 = (light[:, j].double()[:, None, None] for j in range(3))
    ll = l0 * l0
    ll = ll + l1 * l1
    ll = ll + l2 * l2
    dot = g0 * l0
    dot = dot + g1 * l1
    dot = dot + g2 * l2
    den = nn.sqrt() * ll.sqrt()
    ok = den > 0
    safe = torch.where(ok, den, torch.ones_like(den))
    if light is None:
        cosv = torch.where(ok, dot.abs() / safe, torch.zeros_like(den))
    else:
        c = -dot / safe                                                                       # n . l / |l| with n = -g / |g|
        cosv = torch.where(ok & (c > 0), c, torch.zeros_like(den))                            # (NaN > 0 is False)

    def ratio(pair):
        if pair is None:
            return torch.ones_like(den)
        open_, total = pair[0].double(), pair[1].double()
        some = total > 0
        return torch.where(some, open_ / torch.where(some, total, torch.ones_like(total)), torch.ones_like(total))

    amb = float(torch.tensor(ambient, dtype=torch.float32))
    lit_ambient = amb * ratio(ao)
    lit_direct = (1.0 - amb) * cosv
    lit_direct = lit_direct * ratio(shadow)
    shade_ = lit_ambient + lit_direct
    alb = torch.full_like(g, float(GREY)) if albedo is None else albedo.double()
    out = torch.floor(alb * shade_[..., None] + 0.5).clamp(0, 255).to(torch.uint8)
    return torch.where(hit[..., None] != 0, out, torch.tensor(background, dtype=torch.uint8).expand_as(out))


def shade_lit(hit, cam2world, albedo=None, light=None, ao=None, shadow=None, background=(255, 255, 255), ambient=0.3):
    """``shade``'s 'lambert' frames with a directional light, ambient occlusion and shadows, each optional: uint8 [V, H, W, 3].  ``light`` [3] or
    [V, 3] is the WORLD-space direction towards the light (``world_light`` makes it from a camera-space one); ``ao`` and ``shadow`` are the
    ``(open, total)`` pairs of ``occlusion`` [V, H, W].  With g the density gradient, in float64 and in this order:

    cos    with a light v: max(0, -(g . v) / (|g| |v|)) — the normal is n = -g / |g|, the side of the surface that faces the light; without one
           ``shade``'s headlight |g . f| / (|g| |f|); 0 where the denominator is 0 (no normal, or no light direction);
    ao     ao_total > 0 ? ao_open / ao_total : 1, and 1 without the pair; sh the same from the shadow pair;
    shade  (ambient * ao) + (((1 - ambient) * cos) * sh); byte = floor(albedo * shade + 0.5) clamped.

    A gradient with a non-finite component counts as the zero gradient; ``background`` where ``hit.hit`` is 0.  With no light and no pair
    the bytes are ``shade(..., mode='lambert')``'s.  Device tensors run ``p3d_surface_shade_lit``, CPU tensors the definition: the same bytes."""
    h, g, cams, albedo, bg = _shade_operands('surface.shade_lit', hit, cam2world, albedo, background)
    n, height, width = h.shape
    dev = h.device
    if light is not None:
        light = torch.as_tensor(light, dtype=torch.float32).detach()
        light = (light[None].expand(n, -1) if light.ndim == 1 else light).to(dev).contiguous()
        if tuple(light.shape) != (n, 3):
            raise ValueError(f'surface.shade_lit: light must be [3] or [{n}, 3], got {tuple(light.shape)}')
    pairs = []
    for name, pair in (('ao', ao), ('shadow', shadow)):
        if pair is not None:
            pair = tuple(torch.as_tensor(t).detach().to(device=dev, dtype=torch.uint8).contiguous() for t in pair)
            if len(pair) != 2 or any(tuple(t.shape) != (n, height, width) for t in pair):
                raise ValueError(f'surface.shade_lit: {name} must be an (open, total) pair of uint8 [{n}, {height}, {width}]')
        pairs.append(pair)
    if not h.is_cuda:
        return _shade_lit_cpu(h, g, albedo, cams, light, pairs[0], pairs[1], ambient, bg)
    rgb = torch.empty([n, height, width, 3], dtype=torch.uint8, device=dev)
    counts = [_lib.ptr(t) for pair in pairs for t in (pair if pair is not None else (None, None))]
    _lib.check(_lib.lib().p3d_surface_shade_lit(_lib.ptr(h), _lib.ptr(g), _lib.ptr(albedo), _lib.ptr(cams), _lib.ptr(light), *counts, n, height, width,
                                                float(ambient), *bg, _lib.ptr(rgb), _lib.stream_of(rgb)), 'surface_shade_lit')
    return rgb


# ---- frames -------------------------------------------------------------------------------------------------------------------
_CAST_ONLY = ('near', 'far', 'steps', 'refine', 'eps')      # cast's own arguments; the second ray stage shares the rest (threshold, clip_box, planes, ...)


@torch.no_grad()
def render(G, ws, cameras, resolution=512, color='grey', palette=None, background=(255, 255, 255), ambient=0.3, return_hit=False, ao=0, shadows=0,
           light=None, light_space='camera', light_spread=0.0, ao_reach=None, ao_steps=16, shadow_steps=64, occlusion_offset=None, **cast_kwargs):
    """Geometry frames uint8 [V, R, R, 3] of the latent ``ws`` [1, num_ws, w_dim] at ``cameras`` [V, 25]: ``cast`` then ``shade``.

    color  'grey': uniform ``mesh.GREY`` under the headlight; 'normal': the normal map; 'rgb': the decoder's own colour at the hit
           positions (``texture.vertex_rgb``) under the headlight; 'label': the label colour there (``mesh.vertex_labels`` with
           ``palette``).  'rgb' and 'label' query ``G.sample_mixed`` at the hit positions, which runs the backbone once more.
    ``cast_kwargs`` go to ``cast``.  With ``return_hit`` also the ``SurfaceHit``.

    Lighting (all off by default: the path and the bytes above); any of it replaces ``shade`` by ``shade_lit`` (not for the normal map):
    light    a 3-vector, the direction towards a directional light, in ``light_space`` 'camera' (x right, y down, z forward; rotated by
             every camera's cam2world, so the light moves with the camera) or 'world'.  None: the headlight;
    ao       the number of ``sphere_directions`` of the ambient-occlusion stage, 0 for none (about half of them face any pixel; 16 shows
             banding, 64 is smooth): rays of ``ao_steps`` samples up to ``ao_reach``, default box_warp / 4 — a cavity wider than that reads
             as open, and the sample spacing stays near the cast's own;
    shadows  the number of rays towards the light, 0 for none; 1 is a hard shadow, more are spread over the cone of half-angle
             ``light_spread`` radians (``light_directions``).  ``shadow_steps`` samples up to the box diagonal box_warp sqrt 3, beyond
             which nothing can block.  Needs a ``light`` (ValueError): the headlight's shadows fall behind what casts them;
    occlusion_offset  how far along the normal both kinds of ray start off the surface, default box_warp / 128 (``occlusion``)."""
    if color not in ('grey', 'normal', 'rgb', 'label'):
        raise ValueError(f"surface.render: color must be 'grey', 'normal', 'rgb' or 'label', got {color!r}")
    ao, shadows = int(ao), int(shadows)
    if ao < 0 or shadows < 0:
        raise ValueError(f'surface.render: ao and shadows are counts of rays (0: off), got {ao} and {shadows}')
    if shadows > 0 and light is None:
        raise ValueError('surface.render: shadows need a light= direction (a headlight casts no visible shadow)')
    lit = (ao > 0 or shadows > 0 or light is not None) and color != 'normal'
    cameras = torch.as_tensor(cameras, dtype=torch.float32).to(ws.device)
    if lit and (ao > 0 or shadows > 0) and cast_kwargs.get('planes') is None and shape._lattice_reason(G, ws) is None:
        cast_kwargs['planes'] = shape._planes(G, ws, noise_mode=cast_kwargs.get('noise_mode', 'const'))      # one backbone pass for the ray stages
    hit = cast(G, ws, cameras, resolution, **cast_kwargs)
    albedo = None
    if color in ('rgb', 'label'):
        pts = hit.position.reshape(-1, 3)
        colors = texture.vertex_rgb(G, ws, pts) if color == 'rgb' else mesh.vertex_labels(G, ws, pts, palette)[1]
        albedo = colors.reshape(hit.position.shape)
    if not lit:
        frames = shade(hit, cameras[:, :16], albedo, 'normal' if color == 'normal' else 'lambert', background, ambient)
        return (frames, hit) if return_hit else frames
    box = float(G.rendering_kwargs['box_warp'])
    stage = {k: v for k, v in cast_kwargs.items() if k not in _CAST_ONLY}
    stage['offset'] = occlusion_offset
    towards = None if light is None else world_light(light, cameras[:, :16], light_space)
    ao_pair = sh_pair = None
    if ao > 0:
        ao_pair = occlusion(G, ws, hit, sphere_directions(ao), box / 4 if ao_reach is None else ao_reach, steps=ao_steps, **stage)
    if shadows > 0:
        sh_pair = occlusion(G, ws, hit, light_directions(towards, shadows, light_spread), box * math.sqrt(3.0), steps=shadow_steps, **stage)
    frames = shade_lit(hit, cameras[:, :16], albedo, towards, ao_pair, sh_pair, background, ambient)
    return (frames, hit) if return_hit else frames


@torch.no_grad()
def geometry_video(G, ws, cfg='seg2cat', n_frames=120, views_per_step=4, resolution=512, color='grey', path=None, fps=60, gif='pil', format='gif',
                   psnr=None, ssim=None, size=None, resample='lanczos', ms_ssim=None, **render_kwargs):
    """The geometry turntable of ``ws`` [1, num_ws, w_dim]: ``render`` over ``views.video_cameras(G, cfg, n_frames)``, ``views_per_step``
    cameras per cast launch, the backbone run once for all of them where the cast kernel serves.  uint8 [n_frames, R, R, 3] on ws's
    device; with ``path`` also written as a GIF: ``gif='pil'`` through ``mesh.save_gif``, ``gif='device'`` through ``video.save_gif`` (one palette for the
    clip, made and applied on the frames' device).  ``format='avi'``: a true-colour Motion-JPEG AVI through ``video.save_avi`` instead, encoded on the
    frames' device (``gif`` plays no part) — with ``psnr``, ``ssim`` or ``ms_ssim`` (one of them) at the quality that ``video.jpeg_quality_for`` picks for that target;
    ``format='apng'``: a lossless animated PNG through ``video.save_apng``, likewise.  ``size`` ((width, height) or an int): the frames are resized on their
    device first (``resample.resize`` with the filter ``resample``), before the writer and any quality search, and come back at that size."""
    from .video.clip import check_clip_options, save_clip
    check_clip_options('geometry_video', gif, format, psnr, ssim, ms_ssim)
    views._check_resample('geometry_video', size, resample)
    step = int(views_per_step)
    if step < 1:
        raise ValueError(f'geometry_video: views_per_step must be >= 1, got {views_per_step}')
    cameras = views.video_cameras(G, cfg, n_frames).to(ws.device)
    kw = dict(render_kwargs)
    if kw.get('planes') is None and shape._lattice_reason(G, ws) is None:
        kw['planes'] = shape._planes(G, ws, noise_mode=kw.get('noise_mode', 'const'))
    frames = [render(G, ws, cameras[s:s + step], resolution, color=color, **kw) for s in range(0, cameras.shape[0], step)]
    out = torch.cat(frames) if frames else torch.empty([0, int(resolution), int(resolution), 3], dtype=torch.uint8, device=ws.device)
    if size is not None:
        out = resize(out, size, resample)
    if path is not None:
        save_clip(path, out, fps=fps, format=format, gif=gif, psnr=psnr, ssim=ssim, ms_ssim=ms_ssim, who='geometry_video')
    return out
