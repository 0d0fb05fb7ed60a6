"""Colour an extracted mesh from rendered views: area-weighted vertex normals and per-vertex colours baked from frames.

``mesh.extract_mesh`` hands over label colours (or nothing).  Here the views of ``views.render_views`` — the appearance the generator
synthesises — are projected back onto the vertices: a ``Pinhole`` projection lines up pixel for pixel with ``G.synthesis`` at the same
camera label (include/p3d_hip.h), ``mesh.project`` / ``mesh.rasterize`` give the visibility buffer of the mesh for those cameras, and
every vertex takes the weighted mean of the frames it is visible in.

    v, f, colors, seen, frames = texture.textured_mesh(G, ws, 'seg2cat', path='cat.ply')

* ``vertex_normals``: the normalised fp64 sum of a vertex's face cross products, in ascending (face id, corner) order.
* ``bake_accumulate`` / ``bake_finish``: the two steps of a bake on given buffers; ``bake_colors``: project, rasterize and accumulate in
  groups of views (``mesh._view_groups`` / ``mesh._raster_group``, as every loop over views), then finish.  Device tensors run
  csrc/mesh_bake.hip, CPU tensors the formulation below, written operation by operation: it is the definition (include/p3d_hip.h,
  "mesh baking"), and the kernels' bytes equal it.
* ``vertex_rgb``: the decoder's own colour at the vertices, the fallback for vertices no view sees.
* ``bake_cameras`` / ``bake_views`` / ``textured_mesh``: the generator's video cameras, their frames baked onto a mesh, and the whole
  of ``mesh.extract_mesh`` with baked colours.

Per-vertex colours only; a UV atlas and a texture image baked by these same two steps are ``pix2pix3d_amd.atlas``.
"""
import math

import numpy as np
import torch

from . import _lib, mesh, views

GREY = mesh.GREY


def _sqrt(x):
    """The IEEE (correctly rounded) square root of a CPU float64 tensor.  ``torch.sqrt`` is not: its vectorised CPU kernel lands one ulp
    off for about one argument in seventy; numpy's takes the processor's own square-root instruction.  The kernels correct the
    device's fp64 sqrt to the same value (csrc/mesh_bake.hip: sqrt_rn)."""
    return torch.from_numpy(np.sqrt(x.numpy()))


# ---- vertex normals ---------------------------------------------------------------------------------------------------------
def _corner_lists(faces, n_vertices):
    """The CSR of include/p3d_hip.h: (corner_face int64 [3T], the face of every corner, grouped by vertex in ascending (face id,
    corner) order; offsets int64 [V + 1])."""
    flat = faces.reshape(-1)
    sorted_vertex, order = torch.sort(flat, stable=True)                   # ascending position 3 t + corner inside a vertex
    offsets = torch.searchsorted(sorted_vertex, torch.arange(n_vertices + 1, device=faces.device))
    return torch.div(order, 3, rounding_mode='floor'), offsets


def _normals_cpu(vertices, faces, corner_face, offsets):
    v64 = vertices.double()
    p0, p1, p2 = v64[faces[:, 0]], v64[faces[:, 1]], v64[faces[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    face_normal = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],   # separate torch ops: both products rounded
                               e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                               e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], dim=1)
    counts = offsets[1:] - offsets[:-1]
    acc = torch.zeros([vertices.shape[0], 3], dtype=torch.float64)
    live = torch.arange(vertices.shape[0])
    for j in range(int(counts.max()) if len(counts) else 0):               # the j-th corner of every vertex that has one
        live = live[counts[live] > j]
        acc[live] += face_normal[corner_face[offsets[live] + j]]
    x, y, z = acc.unbind(1)
    nn = x * x
    nn = nn + y * y
    nn = nn + z * z
    length = _sqrt(nn)
    ok = (length > 0) & torch.isfinite(length)
    unit = acc / torch.where(ok, length, torch.ones_like(length))[:, None]
    return torch.where(ok[:, None], unit, torch.zeros_like(unit)).float()


def vertex_normals(vertices, faces):
    """float32 [V, 3] area-weighted vertex normals: per vertex the fp64 sum of cross(p1 - p0, p2 - p0) over its faces' corners in
    ascending (face id, corner) order, divided by its length and rounded once; (0, 0, 0) for a vertex without faces or with a zero
    sum.  The sign follows the faces' winding.  Device tensors run p3d_mesh_vertex_normals (the corner lists come from a stable
    torch.sort), CPU tensors the formulation; the bytes are the same."""
    vertices = mesh._mesh_vertices('vertex_normals', vertices)
    nv, dev = vertices.shape[0], vertices.device
    faces = mesh._mesh_faces('vertex_normals', faces, nv).to(dev)
    corner_face, offsets = _corner_lists(faces, nv)
    if not vertices.is_cuda:
        return _normals_cpu(vertices, faces, corner_face, offsets)
    normals = torch.empty([nv, 3], dtype=torch.float32, device=dev)
    faces32, corner32, offsets = faces.to(torch.int32), corner_face.to(torch.int32), offsets.contiguous()
    _lib.check(_lib.lib().p3d_mesh_vertex_normals(_lib.ptr(vertices), nv, _lib.ptr(faces32), faces32.shape[0], _lib.ptr(corner32),
                                                  _lib.ptr(offsets), _lib.ptr(normals), _lib.stream_of(vertices)), 'mesh_vertex_normals')
    return normals


def _normals(what, normals, vertices, faces=None):
    """``normals`` as float32 [V, 3] on the vertices' device; None stands for ``vertex_normals`` where the caller names the faces."""
    if normals is None and faces is not None:
        return vertex_normals(vertices, faces)
    normals = torch.as_tensor(normals).detach().to(device=vertices.device, dtype=torch.float32).contiguous()
    if tuple(normals.shape) != (vertices.shape[0], 3):
        raise ValueError(f'{what}: normals must be [{vertices.shape[0]}, 3], got {tuple(normals.shape)}')
    return normals


# ---- baking -----------------------------------------------------------------------------------------------------------------
def _frames(what, images):
    """``images`` as a uint8 tensor [F, H, W, 3] of a size the kernels take."""
    images = torch.as_tensor(images)
    if images.dtype != torch.uint8 or images.ndim != 4 or images.shape[3] != 3:
        raise ValueError(f'{what}: images must be uint8 [F, H, W, 3], got {images.dtype} {tuple(images.shape)}')
    mesh._size(images.shape[1:3])
    return images


def _views(what, images, cam2world, camera):
    """The checked views of a bake: (images uint8 [F, H, W, 3], cam2world [F, 4, 4] on the CPU, the camera with a ``mesh.Pinhole``'s
    intrinsics as [F, 9] on the CPU)."""
    images = _frames(what, images)
    n = images.shape[0]
    c2w = torch.as_tensor(cam2world, dtype=torch.float32).detach().cpu().reshape(-1, 4, 4)
    if c2w.shape[0] != n:
        raise ValueError(f'{what}: {c2w.shape[0]} cameras for {n} frames')
    return images, c2w, mesh._host_camera(what, camera, n)


def _accumulate_cpu(acc, seen, packed, face_id, depth, images, vertices, normals, cams, ortho, tolerance, min_cos, power):
    """include/p3d_hip.h's baking rules, one torch operation per rounding (no contraction), vectorised over the vertices."""
    n, h, w = face_id.shape
    if h < 2 or w < 2:                                                     # no 2 x 2 footprint fits
        return
    p, nrm, c = vertices.double(), normals.double(), cams.double()
    n0, n1, n2 = nrm.unbind(1)
    nn = n0 * n0
    nn = nn + n1 * n1
    nn = nn + n2 * n2
    nlen = _sqrt(nn)
    for f in range(n):
        rec = packed[f].long()
        tx, ty = rec[:, 0] - 128, rec[:, 1] - 128
        c0, r0, fx, fy = tx >> 8, ty >> 8, tx & 255, ty & 255
        ok = (rec[:, 3] == 0) & (c0 >= 0) & (r0 >= 0) & (c0 + 1 <= w - 1) & (r0 + 1 <= h - 1)
        pix = r0.clamp(0, h - 2) * w + c0.clamp(0, w - 2)                  # clamped as the kernel clamps its addresses
        taps = (pix, pix + 1, pix + w, pix + w + 1)
        ids, dep, img = face_id[f].reshape(-1), depth[f].reshape(-1), images[f].reshape(-1, 3).long()
        for t in taps:
            ok &= ids[t] >= 0
        dmin = torch.fmin(torch.fmin(dep[taps[0]], dep[taps[1]]), torch.fmin(dep[taps[2]], dep[taps[3]]))
        z = packed[f][:, 2].contiguous().view(torch.float32)
        ok &= z.double() <= dmin.double() + tolerance
        if ortho:
            d0, d1, d2 = (-c[f, j].expand(len(p)) for j in (2, 6, 10))
        else:
            d0, d1, d2 = c[f, 3] - p[:, 0], c[f, 7] - p[:, 1], c[f, 11] - p[:, 2]
        dot = n0 * d0
        dot = dot + n1 * d1
        dot = dot + n2 * d2
        dd = d0 * d0
        dd = dd + d1 * d1
        dd = dd + d2 * d2
        den = nlen * _sqrt(dd)
        cosv = torch.where(den > 0, dot.abs() / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
        ok &= cosv >= min_cos
        wgt = cosv
        for _ in range(1, power):
            wgt = wgt * cosv
        w00, w01, w10, w11 = (256 - fy) * (256 - fx), (256 - fy) * fx, fy * (256 - fx), fy * fx
        for ch in range(3):
            num = w00 * img[taps[0], ch] + w01 * img[taps[1], ch] + w10 * img[taps[2], ch] + w11 * img[taps[3], ch]      # exact integer
            col = num.double() / 65536.0
            acc[:, ch] = torch.where(ok, acc[:, ch] + wgt * col, acc[:, ch])
        acc[:, 3] = torch.where(ok, acc[:, 3] + wgt, acc[:, 3])
        seen += ok.to(torch.int32)


def _bake_parameters(tolerance, power, min_cos):
    tolerance, min_cos = float(tolerance), float(min_cos)
    if int(power) != power or not 1 <= int(power) <= 8:
        raise ValueError(f'bake: power must be an integer in 1 .. 8, got {power}')
    if not (math.isfinite(tolerance) and tolerance >= 0.0 and math.isfinite(min_cos) and min_cos >= 0.0):
        raise ValueError(f'bake: tolerance and min_cos must be finite and >= 0, got {tolerance}, {min_cos}')
    return tolerance, int(power), min_cos


def bake_buffers(n_vertices, device):
    """(acc float64 [V, 4] zeros, seen int32 [V] zeros): the in/out buffers of ``bake_accumulate``."""
    return torch.zeros([n_vertices, 4], dtype=torch.float64, device=device), torch.zeros([n_vertices], dtype=torch.int32, device=device)


def bake_accumulate(acc, seen, proj, face_id, depth, images, vertices, normals, cam2world, tolerance=0.01, power=2, min_cos=0.1):
    """Add the views of one group to ``acc`` float64 [V, 4] = sums of (w r, w g, w b, w) and ``seen`` int32 [V], in place and in view
    order, so that groups of views chain into exactly the sums of one call.  ``proj`` is the ``mesh.Projection`` of the vertices,
    ``face_id`` / ``depth`` the raster buffers [F, H, W] of the same mesh and cameras, ``images`` uint8 [F, H, W, 3], ``cam2world`` as
    given to ``mesh.project``.  A view counts for a vertex when the vertex is not dropped, its 2 x 2 bilinear footprint lies inside
    the frame on mesh pixels only, its depth is within ``tolerance`` (world units) of the nearest of the four, and
    cos = |n . d| / (|n| |d|) >= ``min_cos`` with d towards the camera; the weight is cos^power (include/p3d_hip.h).  Every input is
    moved to acc's device, which picks the path."""
    tolerance, power, min_cos = _bake_parameters(tolerance, power, min_cos)
    dev = acc.device
    nv = acc.shape[0]
    if acc.dtype != torch.float64 or tuple(acc.shape) != (nv, 4) or seen.dtype != torch.int32 or tuple(seen.shape) != (nv,) or \
            seen.device != dev or not acc.is_contiguous() or not seen.is_contiguous():
        raise ValueError(f'bake_accumulate: acc must be contiguous float64 [V, 4] and seen int32 [V] on one device, got {acc.dtype} '
                         f'{tuple(acc.shape)} and {seen.dtype} {tuple(seen.shape)}')
    images = _frames('bake_accumulate', images)
    n, h, w = images.shape[:3]
    cams = mesh._cameras(cam2world, mesh.Orthographic(1.0, 1.0))           # position and forward axis only: the model does not matter
    if cams.shape[0] != n or tuple(face_id.shape) != (n, h, w) or tuple(depth.shape) != (n, h, w):
        raise ValueError(f'bake_accumulate: {n} frames of {h} x {w} with {cams.shape[0]} cameras, face_id {tuple(face_id.shape)}, '
                         f'depth {tuple(depth.shape)}')
    if tuple(proj.packed.shape) != (n, nv, 4) or tuple(vertices.shape) != (nv, 3) or tuple(normals.shape) != (nv, 3):
        raise ValueError(f'bake_accumulate: the projection is {tuple(proj.packed.shape)}, vertices {tuple(vertices.shape)}, normals '
                         f'{tuple(normals.shape)}: need ({n}, {nv}, 4), ({nv}, 3), ({nv}, 3)')
    if n > 65535:
        raise ValueError(f'bake_accumulate: at most 65535 frames per call, got {n}')
    packed = proj.packed.detach().to(device=dev, dtype=torch.int32).contiguous()
    face_id = face_id.detach().to(device=dev, dtype=torch.int32).contiguous()
    depth = depth.detach().to(device=dev, dtype=torch.float32).contiguous()
    images = images.detach().to(dev).contiguous()
    vertices = vertices.detach().to(device=dev, dtype=torch.float32).contiguous()
    normals = normals.detach().to(device=dev, dtype=torch.float32).contiguous()
    if not acc.is_cuda:
        _accumulate_cpu(acc, seen, packed, face_id, depth, images, vertices, normals, cams, proj.orthographic, tolerance, min_cos, power)
        return
    cams = cams.to(dev)
    _lib.check(_lib.lib().p3d_mesh_bake_accumulate(_lib.ptr(packed), _lib.ptr(face_id), _lib.ptr(depth), _lib.ptr(images), _lib.ptr(vertices),
                                                   _lib.ptr(normals), _lib.ptr(cams), nv, n, int(proj.orthographic), w, h, tolerance, min_cos,
                                                   power, _lib.ptr(acc), _lib.ptr(seen), _lib.stream_of(acc)), 'mesh_bake_accumulate')


def _fallback(fallback, n_vertices, device):
    """(per-vertex uint8 [V, 3] on the device or None, (r, g, b))."""
    if torch.is_tensor(fallback) or isinstance(fallback, np.ndarray):
        t = torch.as_tensor(fallback)
        if t.ndim == 2:
            if t.dtype != torch.uint8 or tuple(t.shape) != (n_vertices, 3):
                raise ValueError(f'bake_finish: a per-vertex fallback must be uint8 [{n_vertices}, 3], got {t.dtype} {tuple(t.shape)}')
            return t.detach().to(device).contiguous(), (0, 0, 0)
        fallback = t.reshape(-1).tolist()
    rgb = tuple(int(x) for x in fallback)
    if len(rgb) != 3 or not all(0 <= x <= 255 for x in rgb):
        raise ValueError(f'bake_finish: fallback must be uint8 [V, 3] or three values in 0 .. 255, got {fallback!r}')
    return None, rgb


def bake_finish(acc, fallback=(GREY, GREY, GREY)):
    """uint8 [V, 3] from the sums: floor(acc.rgb / acc.w + 0.5) clamped to 255 where acc.w > 0, elsewhere ``fallback`` (uint8 [V, 3] or
    one RGB triple)."""
    nv, dev = acc.shape[0], acc.device
    if acc.dtype != torch.float64 or tuple(acc.shape) != (nv, 4):
        raise ValueError(f'bake_finish: acc must be float64 [V, 4], got {acc.dtype} {tuple(acc.shape)}')
    acc = acc.contiguous()
    per_vertex, rgb = _fallback(fallback, nv, dev)
    if not acc.is_cuda:
        wsum = acc[:, 3]
        have = wsum > 0
        q = torch.floor(acc[:, :3] / torch.where(have, wsum, torch.ones_like(wsum))[:, None] + 0.5)
        mean = torch.where(q >= 0, q.clamp(max=255.0), torch.zeros_like(q)).to(torch.uint8)        # (NaN -> 0)
        other = per_vertex if per_vertex is not None else torch.tensor(rgb, dtype=torch.uint8).expand(nv, 3)
        return torch.where(have[:, None], mean, other)
    colors = torch.empty([nv, 3], dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().p3d_mesh_bake_finish(_lib.ptr(acc), nv, _lib.ptr(per_vertex), *rgb, _lib.ptr(colors), _lib.stream_of(acc)),
               'mesh_bake_finish')
    return colors


@torch.no_grad()
def bake_colors(vertices, faces, images, cam2world, camera, normals=None, tolerance=0.01, power=2, min_cos=0.1,
                fallback=(GREY, GREY, GREY), max_bytes=1 << 30, return_seen=False):
    """Per-vertex colours uint8 [V, 3] of the mesh (vertices float32 [V, 3], faces [T, 3]) from ``images`` uint8 [F, H, W, 3], frames of
    the cameras ``cam2world`` [F, 4, 4] / ``camera`` (``mesh.Orthographic`` or ``mesh.Pinhole``, as for ``mesh.render``): every vertex
    takes the cos^power-weighted mean of the bilinear samples of the frames that see it (``bake_accumulate``), a vertex no frame sees
    takes ``fallback`` (uint8 [V, 3] or one RGB triple).  ``normals`` default to ``vertex_normals``.  ``tolerance`` is the slack of the
    depth test in world units; the default 0.01 is about eight pixels of a 512^2 frame of the unit box (a pixel is 1 / 512 of it, and
    a surface seen at a grazing angle changes depth by several pixels' worth across one footprint).  With ``return_seen`` also int32
    [V], the number of frames that counted.  The views go through project / rasterize / accumulate in groups whose projections take
    at most ``max_bytes`` (as ``mesh.render`` groups them); the result does not depend on the grouping.  Everything runs on the
    vertices' device: csrc/mesh_bake.hip for device tensors, the CPU formulation otherwise, with the same bytes."""
    _bake_parameters(tolerance, power, min_cos)
    vertices = mesh._mesh_vertices('bake_colors', vertices)
    nv, dev = vertices.shape[0], vertices.device
    faces32 = mesh._mesh_faces('bake_colors', faces, nv).to(device=dev, dtype=torch.int32)
    images, c2w, camera = _views('bake_colors', images, cam2world, camera)
    size = tuple(images.shape[1:3])
    images = images.detach().to(dev).contiguous()
    normals = _normals('bake_colors', normals, vertices, faces32)
    acc, seen = bake_buffers(nv, dev)
    for part, poses, cam in mesh._view_groups('bake_colors', c2w, camera, nv, max_bytes) if nv else ():
        proj, face_id, depth = mesh._raster_group(vertices, faces32, poses, cam, size)
        bake_accumulate(acc, seen, proj, face_id, depth, images[part], vertices, normals, poses, tolerance, power, min_cos)
        del proj, face_id, depth
    colors = bake_finish(acc, fallback)
    return (colors, seen) if return_seen else colors


# ---- the generator's own colours and views -----------------------------------------------------------------------------------
@torch.no_grad()
def vertex_rgb(G, ws, vertices, max_batch=10_000_000):
    """uint8 [V, 3] on the vertices' device: the decoder's own colour at the vertices, channels 0..2 of ``G.sample_mixed(...)['rgb']``
    (in chunks of max_batch points) through the ray-marcher's ``* 2 - 1`` (ray_marcher.py:30) and the float -> uint8 rule
    ``views.finish_frames`` applies to images.  Built like ``mesh.vertex_labels``; the colour of a vertex no view sees."""
    pts = vertices.detach().to(device=ws.device, dtype=torch.float32)[None]
    nv = pts.shape[1]
    out = torch.empty([1, 1, nv, 3], dtype=torch.uint8, device=ws.device)
    for head in range(0, nv, max_batch):
        rgb = G.sample_mixed(pts[:, head:head + max_batch], None, ws, truncation_psi=1, noise_mode='const')['rgb'][0, :, :3].float() * 2 - 1
        views.frame_finish([views.FrameJob(rgb.t()[None, :, None, :], out[:, :, head:head + max_batch])])       # [1, 3, 1, n] -> [1, 1, n, 3]
    return out[0, 0].to(vertices.device)


def bake_cameras(G, cfg='seg2cat', n_views=24):
    """float32 [n_views, 25] camera labels: ``views.video_cameras(G, cfg, n_views)``, the poses the generator was trained to render —
    the frontal range for seg2cat / seg2face / edge2cat, the full orbit for edge2car."""
    return views.video_cameras(G, cfg, n_views)


def _generator_views(G, ws, cfg, n_views, jitter, render_kwargs):
    """The views a bake of the generator's appearance takes: (the dict of ``views.render_views`` at ``bake_cameras(G, cfg, n_views)`` —
    the script's ray resolution and noise_mode='const' unless ``render_kwargs`` says otherwise —, cam2world [F, 4, 4], the ``mesh.Pinhole``
    of the labels' intrinsics)."""
    cams = bake_cameras(G, cfg, n_views).to(ws.device)
    render_kwargs = dict(render_kwargs or {})
    render_kwargs.setdefault('noise_mode', 'const')
    render_kwargs.setdefault('neural_rendering_resolution', views.VIDEO_CFG[cfg]['neural_rendering_resolution'])
    frames = views.render_views(G, ws, cams, jitter=jitter, **render_kwargs)
    return frames, cams[:, :16].reshape(-1, 4, 4), mesh.Pinhole(cams[:, 16:25])


@torch.no_grad()
def bake_views(G, ws, vertices, faces, cfg='seg2cat', n_views=24, jitter='frozen', return_frames=False, render_kwargs=None, **bake_kwargs):
    """Bake ``n_views`` views of the latent ``ws`` onto the mesh: ``views.render_views`` at ``bake_cameras(G, cfg, n_views)`` (the
    script's ray resolution and noise_mode='const' unless ``render_kwargs`` says otherwise), then ``bake_colors`` with
    ``mesh.Pinhole(cameras[:, 16:25])`` and ``return_seen=True``; the fallback, unless given, is ``vertex_rgb``.  Returns
    (colors uint8 [V, 3], seen int32 [V]) on the vertices' device, and with ``return_frames`` also the dict of ``render_views``."""
    frames, c2w, camera = _generator_views(G, ws, cfg, n_views, jitter, render_kwargs)
    if 'fallback' not in bake_kwargs:
        bake_kwargs['fallback'] = vertex_rgb(G, ws, vertices)
    bake_kwargs['return_seen'] = True
    colors, seen = bake_colors(vertices, faces, frames['image'], c2w, camera, **bake_kwargs)
    return (colors, seen, frames) if return_frames else (colors, seen)


@torch.no_grad()
def textured_mesh(G, ws, cfg='seg2cat', resolution=512, threshold=50., n_frames=120, image_size=512, keep=None, min_faces=1, cell=None,
                  n_views=24, jitter='frozen', path=None, bake_kwargs=None, smooth=0, tolerance=None, target_faces=None, **synthesis_kwargs):
    """``mesh.extract_mesh`` with the generator's appearance: its geometry and clean-up arguments (``resolution`` .. ``cell``, or ``tolerance`` or ``target_faces`` in its place), colours
    baked from ``n_views`` views (``bake_views``; ``bake_kwargs`` go to ``bake_colors``), the script's turntable rendered with them,
    and, with ``path``, the PLY with colours and vertex normals.  ``smooth`` Taubin iterations (``mesh.smooth`` at its defaults) move
    the vertices right after the clean-up: the bake, the normals, the turntable and the file are the smoothed mesh's.  Works for every
    generator, label channels or not.  Returns
    (vertices, faces, colors uint8 [V, 3], seen int32 [V], frames uint8 [n_frames, image_size, image_size, 3])."""
    vertices, faces = mesh._clean_geometry(G, ws, resolution, threshold, keep, min_faces, cell, tolerance, target_faces, **synthesis_kwargs)
    if smooth and len(vertices):
        vertices = mesh.smooth(vertices, faces, smooth)
    render_kwargs = dict(synthesis_kwargs)
    normals = vertex_normals(vertices, faces)
    colors, seen = bake_views(G, ws, vertices, faces, cfg, n_views, jitter, render_kwargs=render_kwargs, normals=normals, **(bake_kwargs or {}))
    poses, camera = mesh.script_turntable(G, n_frames)
    frames = mesh.render(vertices, faces, poses, camera, image_size, colors=colors)
    if path is not None:
        mesh.write_ply(path, vertices, faces, colors, normals=normals)
    return vertices, faces, colors, seen, frames
