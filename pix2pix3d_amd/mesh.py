"""Render and export extracted meshes (applications/extract_mesh.py:196-262): what the script does with trimesh, pyrender and imageio.

* ``project`` / ``rasterize`` / ``shade``: the three stages of a render.  Device tensors run csrc/mesh_raster.hip (p3d_mesh_project, a
  screen-tiled rasterizer with an LDS z-buffer, p3d_mesh_shade); CPU tensors run the vectorised restatement below, which the kernels
  are tested against.  Every convention (cameras, fixed point, top-left fill rule, fp64 depth, the z-test key) is include/p3d_hip.h's.
* ``render``: the three stages over a batch of frames, the role of pyrender.OffscreenRenderer.render.  The shading is a headlight
  Lambert term on interpolated vertex colours, not pyrender's physically based shading with a spot light.
* ``_view_groups`` / ``_raster_group``: how every loop over views (``render``, ``atlas.render_textured``, ``texture.bake_colors``,
  ``atlas.bake_texture``) is cut into groups whose projections fit ``max_bytes``, and the raster buffers of the mesh for one group.
* ``turntable_poses``: the script's 120-frame orbit (:240-256), in the OpenCV convention (before its OpenGL column flip).
* ``write_ply`` (trimesh's export), ``save_gif`` (imageio.mimsave, through PIL), ``vertex_labels`` (:196-218).
* ``components`` / ``clean`` / ``simplify``: what a trimesh user does between extraction and export (``mesh.split()``, keep the
  largest part, decimate), on the bare geometry: connected components by union-find, a keep-the-largest filter, vertex-clustering
  decimation (csrc/mesh_ops.hip on device tensors, a restatement on CPU tensors; the rules are include/p3d_hip.h's).
* ``adjacency`` / ``smooth`` / ``smooth_values`` / ``smooth_labels``: the filter stage a trimesh user runs next
  (``trimesh.smoothing.filter_taubin``): neighbour lists and boundary flags from sorts, Taubin smoothing of positions or of any
  per-vertex attribute, majority voting of labels, and smooth shading through ``shade(..., normals=)`` (csrc/mesh_filter.hip on device
  tensors; the CPU formulation is the definition and the bytes are the same).
* ``simplify_to``: ``simplify`` with the cell picked from a tolerance, measured by ``geometry.compare`` (geometry.py).  Quadric-error
  decimation to a face count, which keeps what clustering rounds off, is ``decimate.decimate`` (decimate.py; ``target_faces=`` below).
* ``extract_mesh``: shape.extract_geometry, the optional clean-up and filters, the labels and the turntable in one call.
"""
import functools
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, configs, shape

CAMERA_FLOATS = _lib.P3D_MESH_CAMERA_FLOATS
GREY = _lib.P3D_MESH_GREY      # the albedo of a mesh without colours
MAX_SIZE = 2048                # largest image edge the kernels take
_GUARD = 4096 * 256            # guard band, sub-pixel units
_KEY_BG = torch.iinfo(torch.int64).max
_SCRIPT_PI = 3.14              # the script's turntable writes pi as 3.14 (extract_mesh.py:245-251)


class Orthographic(NamedTuple):
    """pyrender.OrthographicCamera: xmag, ymag are half-extents in world units.  znear / zfar as pyrender's defaults."""
    xmag: float
    ymag: float
    znear: float = 0.05
    zfar: float = 100.0


class Pinhole(NamedTuple):
    """The normalised intrinsics of the 25-float camera label: [3, 3], [F, 3, 3] or [F, 9] (fx, fy, cx, cy, skew are read from it)."""
    intrinsics: object
    znear: float = 0.05
    zfar: float = 100.0


class Projection(NamedTuple):
    """p3d_mesh_project's output: packed int32 [F, V, 4] = (sx, sy, fp32 bits of z, dropped) on the vertices' device."""
    packed: torch.Tensor
    orthographic: bool

    @property
    def xy(self):
        return self.packed[..., :2]

    @property
    def z(self):
        return self.packed[..., 2].contiguous().view(torch.float32)

    @property
    def dropped(self):
        return self.packed[..., 3] != 0

    def to(self, device):
        return Projection(self.packed.to(device), self.orthographic)


def _size(resolution):
    h, w = (resolution, resolution) if isinstance(resolution, int) else (int(resolution[0]), int(resolution[1]))
    if not (1 <= h <= MAX_SIZE and 1 <= w <= MAX_SIZE):
        raise ValueError(f'mesh: image size {h} x {w} outside [1, {MAX_SIZE}]^2')
    return h, w


def _cameras(cam2world, camera):
    """cam2world [F, 4, 4] (or [4, 4]) and a camera model -> the float32 [F, 24] rows of include/p3d_hip.h, on the CPU."""
    c2w = torch.as_tensor(cam2world, dtype=torch.float32).detach().cpu().reshape(-1, 16)
    n = c2w.shape[0]
    cams = torch.zeros([n, CAMERA_FLOATS], dtype=torch.float32)
    cams[:, :16] = c2w
    if isinstance(camera, Orthographic):
        if not (float(camera.xmag) > 0 and float(camera.ymag) > 0):
            raise ValueError(f'mesh: xmag and ymag must be positive, got {camera.xmag}, {camera.ymag}')
        cams[:, 16], cams[:, 17] = float(camera.xmag), float(camera.ymag)
    elif isinstance(camera, Pinhole):
        k = torch.as_tensor(camera.intrinsics, dtype=torch.float32).detach().cpu().reshape(-1, 9).expand(n, 9)
        cams[:, 16], cams[:, 17], cams[:, 18], cams[:, 19], cams[:, 20] = k[:, 0], k[:, 4], k[:, 2], k[:, 5], k[:, 1]
    else:
        raise TypeError(f'mesh: camera must be Orthographic or Pinhole, got {type(camera).__name__}')
    znear, zfar = float(camera.znear), float(camera.zfar)
    if not 0.0 < znear < zfar < math.inf:                                 # depths stay positive: the z-test key orders them as integers
        raise ValueError(f'mesh: need 0 < znear < zfar < inf, got znear={znear}, zfar={zfar}')
    cams[:, 21], cams[:, 22] = znear, zfar
    return cams


# ---- projection -------------------------------------------------------------------------------------------------------------
def _vertices32(what, vertices):
    """vertices as contiguous float32 [V, 3], V < 2^31 - 1: the shape alone (no device-to-host copy; ``_mesh_vertices`` adds finiteness)."""
    vertices = vertices.detach().to(torch.float32).contiguous()
    if vertices.ndim != 2 or vertices.shape[1] != 3 or vertices.shape[0] >= 2 ** 31 - 1:
        raise ValueError(f'{what}: vertices must be [V, 3] with V < 2^31 - 1, got {tuple(vertices.shape)}')
    return vertices


def _project_cpu(vertices, cams, ortho, h, w):
    c = cams.double()
    p = vertices.double()
    col = lambda j: c[:, j:j + 1]                                          # noqa: E731  [F, 1]
    px, py, pz = p[:, 0] - col(3), p[:, 1] - col(7), p[:, 2] - col(11)    # [F, V]
    xc = col(0) * px; xc = xc + col(4) * py; xc = xc + col(8) * pz
    yc = col(1) * px; yc = yc + col(5) * py; yc = yc + col(9) * pz
    zc = col(2) * px; zc = zc + col(6) * py; zc = zc + col(10) * pz
    if ortho:
        u = (xc / col(16) + 1.0) * 0.5
        v = (yc / col(17) + 1.0) * 0.5
    else:
        a = col(16) * xc
        a = a + col(20) * yc
        u = a / zc + col(18)
        v = (col(17) * yc) / zc + col(19)
    sx, sy = u * float(w * 256), v * float(h * 256)
    keep = (zc >= col(21)) & (zc <= col(22)) & (sx >= -_GUARD) & (sx <= w * 256 + _GUARD) & (sy >= -_GUARD) & (sy <= h * 256 + _GUARD)
    zero = torch.zeros_like(sx)
    packed = torch.stack([torch.where(keep, sx, zero).round().to(torch.int32), torch.where(keep, sy, zero).round().to(torch.int32),
                          zc.float().view(torch.int32), (~keep).to(torch.int32)], dim=-1)
    return packed


def project(vertices, cam2world, camera, resolution):
    """Project vertices float32 [V, 3] into F frames (cam2world [F, 4, 4], OpenCV convention): a ``Projection`` with fixed-point screen
    positions (8 sub-pixel bits, round half to even), view depth and drop flags (include/p3d_hip.h)."""
    h, w = _size(resolution)
    vertices = _vertices32('project', vertices)
    cams = _cameras(cam2world, camera)
    ortho = isinstance(camera, Orthographic)
    if not vertices.is_cuda:
        return Projection(_project_cpu(vertices, cams, ortho, h, w), ortho)
    n, v = cams.shape[0], vertices.shape[0]
    cams = cams.to(vertices.device)
    packed = torch.empty([n, v, 4], dtype=torch.int32, device=vertices.device)
    _lib.check(_lib.lib().p3d_mesh_project(_lib.ptr(vertices), v, _lib.ptr(cams), n, int(ortho), w, h, _lib.ptr(packed),
                                           _lib.stream_of(vertices)), 'mesh_project')
    return Projection(packed, ortho)


# ---- rasterization ----------------------------------------------------------------------------------------------------------
def _faces32(faces):
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] >= 2 ** 31 - 1:
        raise ValueError(f'mesh: faces must be [T, 3] with T < 2^31 - 1, got {tuple(faces.shape)}')
    if faces.dtype not in (torch.int32, torch.int64):
        raise TypeError(f'mesh: faces must be int32 or int64, got {faces.dtype}')
    return faces.detach().to(torch.int32).contiguous()


def _setup_cpu(packed, faces):
    """The triangle setup of csrc/mesh_raster.hip (tri_setup) for one frame: packed [V, 4], faces int64 [T, 3] ->
    (drawn bool [T], vertex ids [T, 3] in weight order, x, y int64 [T, 3], z float32 [T, 3], c0, c1, r0, r1 before the box test)."""
    nv = packed.shape[0]
    idx = faces.long()
    ok = ((idx >= 0) & (idx < nv)).all(1)
    idx = idx.clamp(0, max(nv - 1, 0))
    rec = packed[idx]                                                     # [T, 3, 4]
    x, y = rec[..., 0].long(), rec[..., 1].long()
    z = rec[..., 2].contiguous().view(torch.float32)
    ok &= (rec[..., 3] == 0).all(1)
    area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    ok &= area != 0
    perm = torch.where((area < 0)[:, None], torch.tensor([0, 2, 1]), torch.tensor([0, 1, 2]))
    idx, x, y, z = (t.gather(1, perm) for t in (idx, x, y, z))
    return ok, idx, x, y, z


def _bbox(x, y, h, w):
    c0 = ((x.min(1).values - 128 + 255) >> 8).clamp(min=0)
    c1 = ((x.max(1).values - 128) >> 8).clamp(max=w - 1)
    r0 = ((y.min(1).values - 128 + 255) >> 8).clamp(min=0)
    r1 = ((y.max(1).values - 128) >> 8).clamp(max=h - 1)
    return c0, c1, r0, r1


def _owns(dx, dy):
    return (dy < 0) | ((dy == 0) & (dx > 0))


def _weights(x, y, r, c):
    """Edge weights and coverage at pixel centres (r, c); x, y [N, 3] int64 in weight order."""
    px, py = (c << 8) + 128, (r << 8) + 128
    dx0, dy0 = x[:, 2] - x[:, 1], y[:, 2] - y[:, 1]
    dx1, dy1 = x[:, 0] - x[:, 2], y[:, 0] - y[:, 2]
    dx2, dy2 = x[:, 1] - x[:, 0], y[:, 1] - y[:, 0]
    w0 = dx0 * (py - y[:, 1]) - dy0 * (px - x[:, 1])
    w1 = dx1 * (py - y[:, 2]) - dy1 * (px - x[:, 2])
    w2 = dx2 * (py - y[:, 0]) - dy2 * (px - x[:, 0])
    inside = ((w0 > 0) | ((w0 == 0) & _owns(dx0, dy0))) & ((w1 > 0) | ((w1 == 0) & _owns(dx1, dy1))) & \
             ((w2 > 0) | ((w2 == 0) & _owns(dx2, dy2)))
    return w0, w1, w2, inside


def _depth(w0, w1, w2, z, ortho):
    """include/p3d_hip.h's depth, in its operation order (separate torch ops: no contraction)."""
    a, b, c = w0.double(), w1.double(), w2.double()
    z0, z1, z2 = (z[:, k].double() for k in range(3))
    s = a + b
    s = s + c
    if ortho:
        n = a * z0
        n = n + b * z1
        n = n + c * z2
        return (n / s).float()
    q = a / z0
    q = q + b / z1
    q = q + c / z2
    return (s / q).float()


def _raster_cpu_frame(packed, faces, ortho, h, w, chunk_pairs=1 << 23):
    ok, _, x, y, z = _setup_cpu(packed, faces)
    c0, c1, r0, r1 = _bbox(x, y, h, w)
    ok &= (c0 <= c1) & (r0 <= r1)
    tid = ok.nonzero()[:, 0]
    nc, nr = (c1 - c0 + 1)[tid], (r1 - r0 + 1)[tid]
    pairs = nc * nr
    keys = torch.full([h * w], _KEY_BG, dtype=torch.int64)
    ends = torch.cumsum(pairs, 0)
    start = 0
    while start < len(tid):                                                # chunks of at most ~chunk_pairs candidate pairs
        base = int(ends[start - 1]) if start else 0
        stop = max(int(torch.searchsorted(ends, base + chunk_pairs, right=True)), start + 1)
        sel = torch.arange(start, stop)
        cnt = pairs[sel]
        rep = torch.repeat_interleave(sel, cnt)
        local = torch.arange(int(cnt.sum())) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
        t = tid[rep]
        r = r0[t] + local // nc[rep]
        c = c0[t] + local % nc[rep]
        w0, w1, w2, inside = _weights(x[t], y[t], r, c)
        t, r, c = t[inside], r[inside], c[inside]
        d = _depth(w0[inside], w1[inside], w2[inside], z[t], ortho)
        key = (d.view(torch.int32).long() << 32) | t
        keys.scatter_reduce_(0, r * w + c, key, 'amin')
        start = stop
    bg = keys == _KEY_BG
    face_id = torch.where(bg, torch.tensor(-1, dtype=torch.int64), keys & 0xffffffff).to(torch.int32)
    depth = torch.where(bg, torch.tensor(float('inf')), (keys >> 32).to(torch.int32).view(torch.float32))
    return face_id.reshape(h, w), depth.reshape(h, w)


def _raster_device(proj, faces, h, w):
    lib = _lib.lib()
    packed = proj.packed.contiguous()
    n, nv = packed.shape[0], packed.shape[1]
    dev = packed.device
    nf = faces.shape[0]
    tiles = int(lib.p3d_mesh_raster_tiles(w, h))
    counts = torch.empty([n, tiles], dtype=torch.int32, device=dev)
    _lib.check(lib.p3d_mesh_raster_count(_lib.ptr(packed), nv, _lib.ptr(faces), nf, n, w, h, _lib.ptr(counts), _lib.stream_of(packed)),
               'mesh_raster_count')
    inclusive = torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64)
    offsets = (inclusive - counts.reshape(-1)).contiguous()
    total = int(inclusive[-1]) if inclusive.numel() else 0                # the one device-to-host copy: sizes the tile lists
    tile_list = torch.empty([max(total, 1)], dtype=torch.int32, device=dev)
    cursor = torch.empty_like(offsets)
    _lib.check(lib.p3d_mesh_raster_bin(_lib.ptr(packed), nv, _lib.ptr(faces), nf, n, w, h, _lib.ptr(offsets), _lib.ptr(cursor),
                                       _lib.ptr(tile_list), _lib.stream_of(packed)), 'mesh_raster_bin')
    face_id = torch.empty([n, h, w], dtype=torch.int32, device=dev)
    depth = torch.empty([n, h, w], dtype=torch.float32, device=dev)
    _lib.check(lib.p3d_mesh_raster(_lib.ptr(packed), nv, _lib.ptr(faces), n, w, h, int(proj.orthographic), _lib.ptr(counts), _lib.ptr(offsets),
                                   _lib.ptr(tile_list), _lib.ptr(face_id), _lib.ptr(depth), _lib.stream_of(packed)), 'mesh_raster')
    return face_id, depth


def rasterize(proj, faces, resolution):
    """The nearest triangle at every pixel centre of every frame: (face_id int32 [F, H, W], -1 for background; depth float32 [F, H, W],
    +inf for background).  Top-left fill rule, fp64 depth from the exact integer edge weights, smallest (depth, face id) key wins
    (include/p3d_hip.h): the result does not depend on the order of the faces beyond their ids.  Device tensors run the tiled kernels
    and copy one total to the host (not graph-capturable); CPU tensors run the restatement."""
    h, w = _size(resolution)
    faces32 = _faces32(faces)
    if proj.packed.is_cuda:
        return _raster_device(proj, faces32.to(proj.packed.device), h, w)
    out = [_raster_cpu_frame(p, faces32.long(), proj.orthographic, h, w) for p in proj.packed]
    if not out:
        return torch.empty([0, h, w], dtype=torch.int32), torch.empty([0, h, w])
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


# ---- shading ----------------------------------------------------------------------------------------------------------------
def _shade_terms_cpu(f, face_id, proj, vertices, faces, cams, ambient, normals=None):
    """What p3d_mesh_shade works out at every drawn pixel of frame f before the albedo: (pix, the flat pixel indices; t, their faces;
    idx [N, 3], the vertex ids in weight order; b, the three barycentrics; the headlight factor).  With ``normals`` float32 [V, 3] the
    normal is p3d_mesh_shade_smooth's, the barycentric mix of the vertex normals, in place of the face's."""
    _, h, w = face_id.shape
    nf = faces.shape[0]
    verts = vertices.double()
    fid = face_id[f].reshape(-1).long()
    pix = ((fid >= 0) & (fid < nf)).nonzero()[:, 0]
    t = fid[pix]
    ok, idx, x, y, z = _setup_cpu(proj.packed[f], faces[t].long())
    c0, c1, r0, r1 = _bbox(x, y, h, w)
    ok &= (c0 <= c1) & (r0 <= r1)
    pix, t, idx, x, y, z = pix[ok], t[ok], idx[ok], x[ok], y[ok], z[ok]
    r, c = pix // w, pix % w
    w0, w1, w2, _ = _weights(x, y, r, c)
    a0, a1, a2 = w0.double(), w1.double(), w2.double()
    if proj.orthographic:
        s = a0 + a1
        s = s + a2
        b = (a0 / s, a1 / s, a2 / s)
    else:
        q0, q1, q2 = a0 / z[:, 0].double(), a1 / z[:, 1].double(), a2 / z[:, 2].double()
        q = q0 + q1
        q = q + q2
        b = (q0 / q, q1 / q, q2 / q)
    if normals is None:
        e1 = verts[idx[:, 1]] - verts[idx[:, 0]]
        e2 = verts[idx[:, 2]] - verts[idx[:, 0]]
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    else:
        nrm = normals.double()
        n = b[0][:, None] * nrm[idx[:, 0]]
        n = n + b[1][:, None] * nrm[idx[:, 1]]
        n = n + b[2][:, None] * nrm[idx[:, 2]]
        nx, ny, nz = n.unbind(1)
    f0, f1, f2 = (float(cams[f, j].double()) for j in (2, 6, 10))
    nn = nx * nx
    nn = nn + ny * ny
    nn = nn + nz * nz
    ff = f0 * f0
    ff = ff + f1 * f1
    ff = ff + f2 * f2
    dot = nx * f0
    dot = dot + ny * f1
    dot = dot + nz * f2
    den = nn.sqrt() * math.sqrt(ff)
    cosv = torch.where(den > 0, dot.abs() / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
    amb = float(torch.tensor(ambient, dtype=torch.float32))
    return pix, t, idx, b, amb + (1.0 - amb) * cosv


def _shaded_bytes(albedo, shade_):
    return torch.floor(albedo * shade_ + 0.5).clamp(0, 255).to(torch.uint8)


def _shade_cpu(face_id, proj, vertices, faces, cams, ambient, background, albedo, normals=None):
    """The CPU shade of every frame: ``albedo(t, idx, b)`` gives the float64 albedo [N, 3] (or [N, 1]) of the N drawn pixels from
    ``_shade_terms_cpu``'s faces, vertex ids and barycentrics; ``normals`` as there."""
    n, h, w = face_id.shape
    out = torch.empty([n, h, w, 3], dtype=torch.uint8)
    out[:] = torch.tensor(background, dtype=torch.uint8)
    for f in range(n):
        pix, t, idx, b, shade_ = _shade_terms_cpu(f, face_id, proj, vertices, faces, cams, ambient, normals)
        out[f].reshape(-1, 3)[pix] = _shaded_bytes(albedo(t, idx, b), shade_[:, None])
    return out


def _vertex_albedo(colors):
    """The albedo of ``shade``: the barycentric mix of the vertex colours (one torch operation per rounding), or uniform grey."""
    if colors is None:
        return lambda t, idx, b: torch.full([len(t), 1], float(GREY), dtype=torch.float64)
    col = colors.double()

    def albedo(t, idx, b):
        alb = b[0][:, None] * col[idx[:, 0]]
        alb = alb + b[1][:, None] * col[idx[:, 1]]
        alb = alb + b[2][:, None] * col[idx[:, 2]]
        return alb
    return albedo


def _shade_operands(what, face_id, proj, vertices, faces, cam2world, background):
    """What ``shade`` and ``atlas.shade_textured`` (``what``: the one that was called) hand to either path, checked and on face_id's
    device (the kernel gets no host pointer): (face_id int32 [F, H, W], Projection, vertices float32 [V, 3], faces int32 [T, 3], camera
    rows float32 [F, 24], background bytes)."""
    if face_id.ndim != 3:
        raise ValueError(f'{what}: face_id must be [F, H, W], got {tuple(face_id.shape)}')
    n, dev = face_id.shape[0], face_id.device
    face_id = face_id.detach().to(torch.int32).contiguous()
    vertices = vertices.detach().to(device=dev, dtype=torch.float32).contiguous()
    faces32 = _faces32(faces).to(dev)
    packed = proj.packed.detach().to(device=dev, dtype=torch.int32).contiguous()
    if tuple(packed.shape) != (n, vertices.shape[0], 4):
        raise ValueError(f'{what}: the projection is {tuple(packed.shape)}, the buffers and vertices need ({n}, {vertices.shape[0]}, 4)')
    # the camera rows only feed the forward axis here: the model's parameters do not matter
    cams = _cameras(cam2world, Orthographic(1.0, 1.0))
    if cams.shape[0] != n:
        raise ValueError(f'{what}: {cams.shape[0]} cameras for {n} frames')
    return face_id, Projection(packed, proj.orthographic), vertices, faces32, cams.to(dev), tuple(int(v) & 255 for v in background)


def shade(face_id, proj, vertices, faces, cam2world, colors=None, background=(255, 255, 255), ambient=0.3, normals=None):
    """uint8 [F, H, W, 3] frames from the raster buffers: barycentric vertex colours (perspective-correct under a pinhole camera) times
    ambient + (1 - ambient) |n . f| (face normal, camera forward axis); colors uint8 [V, 3] or None for uniform grey; background where
    face_id is -1.  cam2world as given to ``project``.  With ``normals`` float32 [V, 3] (``texture.vertex_normals``; need not be unit)
    the shading is smooth: n is the barycentric mix of the three vertex normals (p3d_mesh_shade_smooth).  Every input is moved to
    face_id's device, which picks the path."""
    face_id, proj, vertices, faces32, cams, bg = _shade_operands('shade', face_id, proj, vertices, faces, cam2world, background)
    if colors is not None:
        colors = torch.as_tensor(colors).detach().to(device=face_id.device, dtype=torch.uint8).contiguous()
        if tuple(colors.shape) != (vertices.shape[0], 3):
            raise ValueError(f'shade: colors must be uint8 [V, 3], got {tuple(colors.shape)}')
    if normals is not None:
        normals = torch.as_tensor(normals)
        if normals.dtype != torch.float32 or tuple(normals.shape) != (vertices.shape[0], 3):
            raise ValueError(f'shade: normals must be float32 [{vertices.shape[0]}, 3], got {normals.dtype} {tuple(normals.shape)}')
        normals = normals.detach().to(face_id.device).contiguous()
    if not face_id.is_cuda:
        return _shade_cpu(face_id, proj, vertices, faces32, cams, ambient, bg, _vertex_albedo(colors), normals)
    n, h, w = face_id.shape
    rgb = torch.empty([n, h, w, 3], dtype=torch.uint8, device=face_id.device)
    if normals is not None:
        _lib.check(_lib.lib().p3d_mesh_shade_smooth(_lib.ptr(face_id), _lib.ptr(proj.packed), _lib.ptr(vertices), vertices.shape[0],
                                                    _lib.ptr(faces32), faces32.shape[0], _lib.ptr(normals), _lib.ptr(colors), _lib.ptr(cams),
                                                    n, int(proj.orthographic), w, h, float(ambient), *bg, _lib.ptr(rgb),
                                                    _lib.stream_of(rgb)), 'mesh_shade_smooth')
        return rgb
    _lib.check(_lib.lib().p3d_mesh_shade(_lib.ptr(face_id), _lib.ptr(proj.packed), _lib.ptr(vertices), vertices.shape[0],
                                         _lib.ptr(faces32), faces32.shape[0], _lib.ptr(colors), _lib.ptr(cams), n, int(proj.orthographic),
                                         w, h, float(ambient), *bg, _lib.ptr(rgb), _lib.stream_of(rgb)), 'mesh_shade')
    return rgb


# ---- groups of views --------------------------------------------------------------------------------------------------------
def _host_camera(what, camera, n_frames):
    """``camera`` for ``n_frames`` frames: a Pinhole with its intrinsics as float32 [F, 9] on the CPU (one set serves every frame),
    another camera as it is."""
    if not isinstance(camera, Pinhole):
        return camera
    k = torch.as_tensor(camera.intrinsics, dtype=torch.float32).detach().cpu().reshape(-1, 9)
    if k.shape[0] not in (1, n_frames):
        raise ValueError(f'{what}: {k.shape[0]} intrinsics for {n_frames} frames')
    return camera._replace(intrinsics=k.expand(n_frames, 9))


def _view_groups(what, cam2world, camera, n_points, max_bytes):
    """The F views cut into groups whose projections of ``n_points`` points (16 bytes per point and view) take at most ``max_bytes``,
    one view at least: a list of (the slice of the frames, their cam2world [G, 4, 4], their camera), poses and intrinsics on the CPU
    (brought there once).  THE place that sizes a group and slices per-frame intrinsics; idempotent on views ``texture._views`` checked."""
    c2w = torch.as_tensor(cam2world, dtype=torch.float32).detach().cpu().reshape(-1, 4, 4)
    n = c2w.shape[0]
    camera = _host_camera(what, camera, n)
    group = max(1, min(n, max_bytes // max(1, 16 * n_points)))
    parts = [slice(s, s + group) for s in range(0, n, group)]
    pinhole = isinstance(camera, Pinhole)
    return [(part, c2w[part], camera._replace(intrinsics=camera.intrinsics[part]) if pinhole else camera) for part in parts]


def _raster_group(vertices, faces32, cam2world, camera, size):
    """(proj, face_id, depth) of the mesh for one group of views.  Not folded into ``_view_groups`` as a generator: its caller decides
    when the projection dies (``atlas._bake`` drops it before it projects the texels), and a suspended generator would keep it."""
    proj = project(vertices, cam2world, camera, size)
    return (proj,) + rasterize(proj, faces32, size)


def _render(what, vertices, faces, cam2world, camera, resolution, shade_stage, return_buffers, max_bytes):
    """``render`` with ``shade_stage(face_id, proj, vertices, faces32, cam2world)`` as the last stage of every group."""
    h, w = _size(resolution)
    vertices = vertices.detach().to(torch.float32).contiguous()
    faces32 = _faces32(faces).to(vertices.device)
    frames, ids, depths = [], [], []
    for _, c2w, cam in _view_groups(what, cam2world, camera, vertices.shape[0], max_bytes):
        proj, face_id, depth = _raster_group(vertices, faces32, c2w, cam, (h, w))
        frames.append(shade_stage(face_id, proj, vertices, faces32, c2w))
        if return_buffers:
            ids.append(face_id)
            depths.append(depth)
        del proj
    out = torch.cat(frames) if frames else torch.empty([0, h, w, 3], dtype=torch.uint8, device=vertices.device)
    if return_buffers:
        return out, torch.cat(ids), torch.cat(depths)
    return out


@torch.no_grad()
def render(vertices, faces, cam2world, camera, resolution=512, colors=None, background=(255, 255, 255), ambient=0.3, return_buffers=False,
           max_bytes=1 << 30, normals=None):
    """The role of pyrender.OffscreenRenderer.render for every pose of cam2world [F, 4, 4] (OpenCV convention): uint8 frames
    [F, H, W, 3] on the vertices' device.  ``camera`` is Orthographic(xmag, ymag) or Pinhole(intrinsics); faces int32 or int64 [T, 3];
    colors uint8 [V, 3] or None (uniform grey); normals float32 [V, 3] or None (flat shading), as for ``shade``.  With
    return_buffers=True also (face_id int32 [F, H, W], depth float32 [F, H, W]).
    Frames go through project / rasterize / shade in groups whose projections take at most ``max_bytes``."""
    if colors is not None:
        colors = torch.as_tensor(colors).to(device=vertices.device, dtype=torch.uint8).contiguous()
    stage = functools.partial(shade, colors=colors, background=background, ambient=ambient, normals=normals)
    return _render('render', vertices, faces, cam2world, camera, resolution, stage, return_buffers, max_bytes)


# ---- cameras ----------------------------------------------------------------------------------------------------------------
def turntable_poses(pivot, radius, n_frames=120, yaw0=_SCRIPT_PI / 2, yaw_range=0.35, pitch_range=0.25, pitch0=_SCRIPT_PI / 2 - 0.05):
    """float32 [n_frames, 4, 4] cam2world, OpenCV convention: frame k is LookAtPoseSampler.sample(yaw0 + yaw_range sin(2 3.14 k / n),
    pitch0 + pitch_range cos(2 3.14 k / n), pivot, radius) as extract_mesh.py:240-256 draws it (before its OpenGL column flip).  As
    in LookAtPoseSampler, the camera lies on the sphere of that radius about the world origin and looks at the pivot.  Defaults: the
    seg2cat / seg2face turntable; edge2car is yaw0=-3.14/2, yaw_range=pi, pitch_range=pi/2 (and radius 1.2)."""
    out = np.empty([n_frames, 4, 4], np.float64)
    for k in range(n_frames):
        h = yaw0 + yaw_range * math.sin(2 * _SCRIPT_PI * k / n_frames)
        v = pitch0 + pitch_range * math.cos(2 * _SCRIPT_PI * k / n_frames)
        v = min(max(v, 1e-5), math.pi - 1e-5)
        phi = math.acos(1 - 2 * (v / math.pi))
        pos = radius * np.array([math.sin(phi) * math.cos(math.pi - h), math.cos(phi), math.sin(phi) * math.sin(math.pi - h)])
        out[k] = configs.look_at(pos, np.asarray(pivot, np.float64))
    return torch.from_numpy(out).to(torch.float32)


# ---- files ------------------------------------------------------------------------------------------------------------------
def write_ply(path, vertices, faces, colors=None, normals=None):
    """Binary little-endian PLY (what trimesh's export writes for the script): vertex float x y z [+ float nx ny nz]
    [+ uchar red green blue], face list uchar int vertex_indices."""
    v = vertices.detach().cpu().to(torch.float32).numpy()
    f = faces.detach().cpu().numpy()
    if f.size and (f.min() < 0 or f.max() >= len(v) or f.max() > np.iinfo(np.int32).max):
        raise ValueError('write_ply: face index outside [0, V)')
    vfields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    props = 'property float x\nproperty float y\nproperty float z\n'
    if normals is not None:
        vfields += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
        props += 'property float nx\nproperty float ny\nproperty float nz\n'
    if colors is not None:
        vfields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
        props += 'property uchar red\nproperty uchar green\nproperty uchar blue\n'
    header = (f'ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\n{props}'
              f'element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n')
    vrec = np.empty(len(v), dtype=vfields)
    vrec['x'], vrec['y'], vrec['z'] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        n = torch.as_tensor(normals).detach().cpu().to(torch.float32).numpy()
        if n.shape != v.shape:
            raise ValueError(f'write_ply: normals must be [V, 3] like the vertices, got {n.shape}')
        vrec['nx'], vrec['ny'], vrec['nz'] = n[:, 0], n[:, 1], n[:, 2]
    if colors is not None:
        c = torch.as_tensor(colors).detach().cpu().to(torch.uint8).numpy()
        vrec['red'], vrec['green'], vrec['blue'] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.empty(len(f), dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    frec['n'] = 3
    frec['i'] = f
    with open(path, 'wb') as fh:
        fh.write(header.encode('ascii'))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def save_gif(path, frames, fps=60):
    """imageio.mimsave(path, frames, fps=fps) through PIL: frames uint8 [F, H, W, 3], looping forever."""
    from PIL import Image
    arr = torch.as_tensor(frames).detach().cpu().to(torch.uint8).numpy()
    images = [Image.fromarray(a) for a in arr]
    images[0].save(path, save_all=True, append_images=images[1:], duration=max(1, round(1000 / fps)), loop=0)


# ---- clean-up: connected components, keep the largest, vertex clustering -------------------------------------------------------
def _mesh_vertices(what, vertices):
    vertices = _vertices32(what, vertices)
    if not bool(torch.isfinite(vertices).all()):
        raise ValueError(f'{what}: vertices must be finite')
    return vertices


def _mesh_faces(what, faces, n_vertices):
    """faces [T, 3], int32 or int64, every index in [0, V) -> int64 (on a device the range check is one device-to-host copy)."""
    n_vertices = int(n_vertices)
    if not 0 <= n_vertices < 2 ** 31 - 1:
        raise ValueError(f'{what}: n_vertices must be in [0, 2^31 - 1), got {n_vertices}')
    _faces32(faces)
    faces = faces.detach().long().contiguous()
    if faces.numel():
        lo, hi = torch.stack(torch.aminmax(faces)).tolist()
        if lo < 0 or hi >= n_vertices:
            raise ValueError(f'{what}: face index outside [0, {n_vertices}) (indices span [{lo}, {hi}])')
    return faces


def _components_cpu(faces, n_vertices):
    """Union-find by rounds: every root an edge joins to a smaller root is hooked under the smallest such root (scatter amin), pointer
    jumping flattens the forest, and the edges that still join two roots go round again.  O(log V) rounds on any mesh."""
    parent = torch.arange(n_vertices, dtype=torch.int64, device=faces.device)
    a = torch.cat([faces[:, 0], faces[:, 1]])                              # (corner 0, corner 2) follows from the other two edges
    b = torch.cat([faces[:, 1], faces[:, 2]])
    while True:
        ra, rb = parent[a], parent[b]
        live = ra != rb
        if not bool(live.any()):
            return parent
        a, b, ra, rb = a[live], b[live], ra[live], rb[live]
        parent.scatter_reduce_(0, torch.maximum(ra, rb), torch.minimum(ra, rb), 'amin')
        while True:
            up = parent[parent]
            if torch.equal(up, parent):
                break
            parent = up


def components(faces, n_vertices):
    """int64 [V] labels: label[v] is the smallest vertex id of v's connected component, two vertices being connected when a face uses
    both (a vertex no face uses is its own component).  A pure function of the inputs: the same for any order of the faces.  Device
    faces run p3d_mesh_components (union-find, three launches); CPU faces run the same rule in vectorised rounds."""
    faces = _mesh_faces('components', faces, n_vertices)
    n_vertices = int(n_vertices)
    if not faces.is_cuda:
        return _components_cpu(faces, n_vertices)
    faces32 = faces.to(torch.int32)
    label = torch.empty([n_vertices], dtype=torch.int32, device=faces.device)
    _lib.check(_lib.lib().p3d_mesh_components(_lib.ptr(faces32), faces32.shape[0], n_vertices, _lib.ptr(label), _lib.stream_of(faces32)),
               'mesh_components')
    return label.long()


def clean(vertices, faces, keep=1, min_faces=1):
    """Keep the largest connected components (the role of trimesh's ``mesh.split()`` and a pick): components are ranked by face
    count, descending, ties to the smaller label; the first ``keep`` of those with at least ``min_faces`` faces survive (keep=None:
    all of them).  Vertices no surviving face uses are dropped; vertex and face order are kept.  Returns (vertices', faces' int64,
    kept int64 [V'] = the original id of every vertex that is left)."""
    if keep is not None and int(keep) < 1:
        raise ValueError(f'clean: keep must be >= 1 or None, got {keep}')
    vertices = _mesh_vertices('clean', vertices)
    nv, dev = vertices.shape[0], vertices.device
    faces = _mesh_faces('clean', faces, nv).to(dev)
    label = components(faces, nv)
    face_label = label[faces[:, 0]]
    # the components that have faces, ascending by label (so a stable sort leaves ties to the smaller label), and their face counts; by
    # sorting, not a histogram: on a device that is atomics, and one large component puts nearly all of them on one word
    roots, count = torch.unique(face_label, return_counts=True)
    rank = torch.sort(count, descending=True, stable=True).indices
    rank = rank[count[rank] >= int(min_faces)]
    if keep is not None:
        rank = rank[:int(keep)]
    alive = torch.zeros([nv], dtype=torch.bool, device=dev)
    alive[roots[rank]] = True
    faces = faces[alive[face_label]]
    used = torch.zeros([nv], dtype=torch.bool, device=dev)
    used[faces.reshape(-1)] = True
    kept = used.nonzero()[:, 0]
    remap = torch.cumsum(used, 0) - 1
    return vertices[kept], remap[faces], kept


def _cluster_keys_cpu(vertices, lo, cell, n):
    top = torch.tensor([k - 1 for k in n], dtype=torch.float64)
    i = torch.floor(torch.div(vertices.double() - lo.double(), torch.tensor(cell, dtype=torch.float64)))      # a true fp64 divide
    i = torch.minimum(i.clamp(min=0.0), top).long()
    return (i[:, 2] * n[1] + i[:, 1]) * n[0] + i[:, 0]


def _cluster_means_cpu(vertices, order, offsets):
    """Per segment of ``order`` the fp64 sum in that order, one member of every segment per pass (as many passes as the fullest
    cell has vertices), the fp64 quotient, one rounding to fp32: p3d_mesh_cluster_means' arithmetic exactly."""
    counts = offsets[1:] - offsets[:-1]
    acc = torch.zeros([len(counts), 3], dtype=torch.float64)
    v64 = vertices.double()
    live = torch.arange(len(counts))
    for j in range(int(counts.max()) if len(counts) else 0):
        live = live[counts[live] > j]
        acc[live] += v64[order[offsets[live] + j]]
    return (acc / counts.double()[:, None]).float()


def simplify(vertices, faces, cell):
    """Vertex-clustering decimation: a grid of cubic cells of edge ``cell`` (in the vertices' units) from the vertices' per-axis
    minimum; every occupied cell becomes one vertex, the mean of its members (fp64 sum in ascending vertex id, rounded once), in
    ascending cell order (z outermost).  Faces are remapped; a face with two corners in one cell is dropped, and of the faces with
    the same three vertices the first in input order stays, with its winding (a thin sheet whose two sides collapse into the same
    cells becomes one single-sided sheet).  Carries no vertex attributes: label the result.  Returns (vertices', faces' int64).
    Device tensors run csrc/mesh_ops.hip's kernels, with the sorts and scans between them in torch and one device-to-host copy of
    the bounding box; CPU tensors run the restatement."""
    cell = float(cell)
    if not (cell > 0.0 and math.isfinite(cell)):
        raise ValueError(f'simplify: cell must be positive and finite, got {cell}')
    vertices = _mesh_vertices('simplify', vertices)
    nv, dev = vertices.shape[0], vertices.device
    faces = _mesh_faces('simplify', faces, nv).to(dev)
    nf = faces.shape[0]
    if nv == 0:
        return vertices, faces
    box = torch.stack([vertices.min(0).values, vertices.max(0).values]).cpu()
    lo = box[0]
    n = (torch.floor(torch.div(box[1].double() - lo.double(), torch.tensor(cell, dtype=torch.float64))) + 1.0).tolist()
    if max(n) > 2 ** 31 - 1 or n[0] * n[1] * n[2] >= 2.0 ** 62:
        raise ValueError(f'simplify: cell {cell} gives {n[0]:.0f} x {n[1]:.0f} x {n[2]:.0f} cells, beyond the 2^62 a key holds')
    n = [int(k) for k in n]
    lib = _lib.lib() if vertices.is_cuda else None
    if lib is None:
        key = _cluster_keys_cpu(vertices, lo, cell, n)
    else:
        key = torch.empty([nv], dtype=torch.int64, device=dev)
        _lib.check(lib.p3d_mesh_cluster_keys(_lib.ptr(vertices), nv, float(lo[0]), float(lo[1]), float(lo[2]), cell, n[0], n[1], n[2],
                                             _lib.ptr(key), _lib.stream_of(vertices)), 'mesh_cluster_keys')
    sorted_key, order = torch.sort(key, stable=True)                       # ascending vertex id inside a cell
    counts = torch.unique_consecutive(sorted_key, return_counts=True)[1]
    nc = counts.shape[0]
    offsets = torch.zeros([nc + 1], dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0)
    cluster = torch.empty([nv], dtype=torch.int64, device=dev)
    cluster[order] = torch.repeat_interleave(torch.arange(nc, device=dev), counts)
    if lib is None:
        means = _cluster_means_cpu(vertices, order, offsets)
    else:
        order32 = order.to(torch.int32)
        means = torch.empty([nc, 3], dtype=torch.float32, device=dev)
        _lib.check(lib.p3d_mesh_cluster_means(_lib.ptr(vertices), nv, _lib.ptr(order32), _lib.ptr(offsets), nc, _lib.ptr(means),
                                              _lib.stream_of(vertices)), 'mesh_cluster_means')
    if nf == 0:
        return means, faces
    if lib is None:
        mapped = cluster[faces]
        triple = mapped.sort(1).values
        degenerate = (triple[:, 0] == triple[:, 1]) | (triple[:, 1] == triple[:, 2])
    else:
        faces32, cluster32 = faces.to(torch.int32), cluster.to(torch.int32)
        mapped, triple = torch.empty_like(faces32), torch.empty_like(faces32)
        flags = torch.empty([nf], dtype=torch.uint8, device=dev)
        _lib.check(lib.p3d_mesh_cluster_faces(_lib.ptr(faces32), nf, nv, _lib.ptr(cluster32), _lib.ptr(mapped), _lib.ptr(triple),
                                              _lib.ptr(flags), _lib.stream_of(faces32)), 'mesh_cluster_faces')
        degenerate = flags != 0
    idx = (~degenerate).nonzero()[:, 0]
    triple = triple[idx].long()
    # one int64 per vertex set: the rank of the first two ids (below T), then the third (below C)
    pair = torch.unique(triple[:, 0] * nc + triple[:, 1], return_inverse=True)[1]
    sorted_set, by_set = torch.sort(pair * nc + triple[:, 2], stable=True)  # input order inside a run of equal sets
    first = torch.ones_like(sorted_set, dtype=torch.bool)
    first[1:] = sorted_set[1:] != sorted_set[:-1]
    keep = torch.sort(idx[by_set[first]]).values
    return means, mapped[keep].long()


SIMPLIFY_RUNGS = 32            # simplify_to's ladder of cells: tolerance / 4 * 2^(i / 4), i = 0 .. 31 (up to about 54 tolerances)


def simplify_to(vertices, faces, tolerance, spacing=None):
    """``simplify`` with its cell picked from a tolerance: (vertices', faces', cell, agreement).  The cell comes from the fixed ladder
    tolerance / 4 * 2^(i / 4), i = 0 .. 31: rung 0 is tried, then a bisection over the rung index in five steps looks for the largest
    rung whose result keeps the sampled symmetric Hausdorff distance to the input (``geometry.compare`` at ``spacing``, default the
    input's diagonal over 512; one device-to-host copy per rung tried, six in all) at or below ``tolerance``.  The distance is NOT
    monotone in the cell (a thin sheet collapses at one cell and not at the next), so the only promise is the post-condition: the
    mesh that comes back met the tolerance as measured, ``agreement`` being that measurement (A = the input), and the next rung, if
    the ladder has one, did not.  If rung 0 fails the input comes back unchanged with cell None (and that rung's agreement, or None where
    the cell was too fine for ``simplify`` to take)."""
    from . import geometry                                                 # (geometry imports this module)
    tolerance = float(tolerance)
    if not (tolerance > 0.0 and math.isfinite(tolerance)):
        raise ValueError(f'simplify_to: tolerance must be positive and finite, got {tolerance}')
    vertices = _mesh_vertices('simplify_to', vertices)
    faces = _mesh_faces('simplify_to', faces, vertices.shape[0]).to(vertices.device)
    spacing = geometry.diagonal(vertices) / 512 if spacing is None else float(spacing)

    def rung(i):
        cell = tolerance / 4 * 2.0 ** (i / 4)
        try:
            v, f = simplify(vertices, faces, cell)
        except ValueError:                                                 # more cells than a key holds: a rung that cannot be taken fails
            return False, (vertices, faces, None, None)
        agreement = geometry.compare(vertices, faces, v, f, spacing, (tolerance,))
        return bool(agreement.hausdorff <= tolerance), (v, f, cell, agreement)

    ok, best = rung(0)
    if not ok:
        return vertices, faces, None, best[3]
    passed, failed = 0, SIMPLIFY_RUNGS
    for _ in range(5):                                                     # 32 rungs: five halvings leave failed = passed + 1
        mid = (passed + failed) // 2
        ok, result = rung(mid)
        if ok:
            passed, best = mid, result
        else:
            failed = mid
    return best


# ---- filtering: adjacency, Taubin smoothing, label voting -----------------------------------------------------------------------
class Adjacency(NamedTuple):
    """The vertex adjacency of an indexed mesh (``adjacency``): the list of v is neighbours[offsets[v]:offsets[v + 1]]."""
    offsets: torch.Tensor          # int64 [V + 1]
    neighbours: torch.Tensor       # int32 [E]
    boundary: torch.Tensor         # bool [V]


def adjacency(faces, n_vertices):
    """``Adjacency`` of the mesh: the list of v holds the distinct vertices w != v that share a face with v, in ascending id;
    boundary[v] says that v is an end of an undirected edge {a, b}, a != b, that exactly one face side uses (an edge three faces share
    is not a boundary edge).  A face lists its three sides; a side a == b of a degenerate face is ignored, so that a face with a
    repeated index adds no self entry and, using its one edge from both sides, no boundary flag of its own.  A pure function of
    (faces, V): face order and corner order do not matter.  Sorts and uniques of int64 keys a * V + b in torch, the same on a device
    and on the CPU: no kernel."""
    faces = _mesh_faces('adjacency', faces, n_vertices)
    nv, dev = int(n_vertices), faces.device
    a = torch.cat([faces[:, 0], faces[:, 1], faces[:, 2]])                 # the three sides of every face
    b = torch.cat([faces[:, 1], faces[:, 2], faces[:, 0]])
    proper = a != b
    a, b = a[proper], b[proper]
    key = torch.unique(torch.cat([a * nv + b, b * nv + a]))                # sorted: by vertex, then by neighbour
    source = torch.div(key, max(nv, 1), rounding_mode='floor')
    offsets = torch.searchsorted(source, torch.arange(nv + 1, device=dev))
    neighbours = (key - source * nv).to(torch.int32)
    edge, uses = torch.unique(torch.minimum(a, b) * nv + torch.maximum(a, b), return_counts=True)
    edge = edge[uses == 1]
    low = torch.div(edge, max(nv, 1), rounding_mode='floor')
    boundary = torch.zeros([nv], dtype=torch.bool, device=dev)
    boundary[low] = True
    boundary[edge - low * nv] = True
    return Adjacency(offsets, neighbours, boundary)


def _filter_adjacency(what, faces, n_vertices, given, device):
    """The ``Adjacency`` a filter works on, on ``device``: ``given`` (checked for its shapes; the kernels skip what lies out of
    range) or ``adjacency(faces, n_vertices)``."""
    if given is None:
        return adjacency(_mesh_faces(what, faces, n_vertices).to(device), n_vertices)
    offsets, neighbours, boundary = given
    if offsets.dtype != torch.int64 or tuple(offsets.shape) != (n_vertices + 1,) or neighbours.dtype != torch.int32 or neighbours.ndim != 1 \
            or boundary.dtype != torch.bool or tuple(boundary.shape) != (n_vertices,):
        raise ValueError(f'{what}: adjacency must be (int64 [{n_vertices + 1}], int32 [E], bool [{n_vertices}]) as mesh.adjacency returns it')
    return Adjacency(offsets.to(device).contiguous(), neighbours.to(device).contiguous(), boundary.to(device))


def _pinned(what, pinned, n_vertices, device, also=None):
    """``pinned`` (bool [V] or None) ORed with ``also`` as the kernels' uint8 [V], or None when nothing is pinned by either."""
    if pinned is not None:
        pinned = torch.as_tensor(pinned)
        if pinned.dtype != torch.bool or tuple(pinned.shape) != (n_vertices,):
            raise ValueError(f'{what}: pinned must be bool [{n_vertices}], got {pinned.dtype} {tuple(pinned.shape)}')
        pinned = pinned.to(device)
        also = pinned if also is None else pinned | also
    return None if also is None else also.to(torch.uint8).contiguous()


def _iterations(what, iterations):
    if isinstance(iterations, bool) or int(iterations) != iterations or iterations < 0:
        raise ValueError(f'{what}: iterations must be a non-negative integer, got {iterations!r}')
    return int(iterations)


def _smooth_step_cpu(x, adj, pinned, factor):
    """p3d_mesh_smooth_step's arithmetic exactly: per vertex the fp64 sum of its list in list order, one list position of every
    vertex per pass (as ``_cluster_means_cpu``), then every rounding its own torch operation.  Once only a few long lists are left
    (the hub of a fan), each is finished entry by entry in Python floats, which are the same fp64 additions in the same order."""
    offsets, neighbours = adj.offsets, adj.neighbours.long()
    counts = offsets[1:] - offsets[:-1]
    x64 = x.double()
    acc = torch.zeros_like(x64)
    live = (counts > 0).nonzero()[:, 0]
    j = 0
    while len(live) > 16:
        acc[live] += x64[neighbours[offsets[live] + j]]
        j += 1
        live = live[counts[live] > j]
    for v in live.tolist():
        total = acc[v].tolist()
        for row in x64[neighbours[offsets[v] + j:offsets[v + 1]]].tolist():
            total = [a + b for a, b in zip(total, row)]
        acc[v] = torch.tensor(total, dtype=torch.float64)
    m = acc / counts.clamp(min=1).double()[:, None]
    d = m - x64
    p = factor * d
    y = x64 + p
    moves = counts > 0
    if pinned is not None:
        moves &= pinned == 0
    return torch.where(moves[:, None], y.float(), x)


def _smooth_steps(x, adj, pinned, factors):
    """One Jacobi step per entry of ``factors`` on x float32 [V, C], the input left as it is and two buffers taking turns (a step
    must not write what it reads)."""
    if not x.is_cuda:
        for factor in factors:
            x = _smooth_step_cpu(x, adj, pinned, float(factor))
        return x
    lib = _lib.lib()
    spare = [torch.empty_like(x), torch.empty_like(x)] if len(factors) > 1 else [torch.empty_like(x)]
    for k, factor in enumerate(factors):
        out = spare[k % 2]
        _lib.check(lib.p3d_mesh_smooth_step(_lib.ptr(x), x.shape[0], x.shape[1], _lib.ptr(adj.offsets), _lib.ptr(adj.neighbours),
                                            adj.neighbours.shape[0], _lib.ptr(pinned), float(factor), _lib.ptr(out), _lib.stream_of(x)),
                   'mesh_smooth_step')
        x = out
    return x


def smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, pinned=None, adjacency=None):
    """Taubin smoothing of the positions (the role of trimesh.smoothing.filter_taubin): float32 [V, 3].  Every iteration is a Jacobi
    step x <- x + lam (mean of the neighbours - x) and then the same step with ``mu`` < -lam, which undoes the shrinkage of the
    first; mu = 0 leaves the second step out (plain Laplacian smoothing, which shrinks).  Uniform weights over ``mesh.adjacency``.
    ``pinned`` bool [V] vertices stay where they are, and with ``pin_boundary`` so do the boundary vertices: a mesh the box cut is
    open, and a free rim shrinks.  The faces are untouched; ``adjacency`` spares building it again.  iterations = 0 returns the
    input's bits.  Device vertices run p3d_mesh_smooth_step, one launch per step; CPU vertices the formulation, with the same bytes
    (fp64 sums in list order, include/p3d_hip.h)."""
    iterations = _iterations('smooth', iterations)
    lam, mu = float(lam), float(mu)
    if not 0.0 < lam <= 1.0:
        raise ValueError(f'smooth: lam must be in (0, 1], got {lam}')
    if not (mu == 0.0 or -math.inf < mu < -lam):
        raise ValueError(f'smooth: mu must be 0 or below -lam = {-lam}, got {mu}')
    vertices = _mesh_vertices('smooth', vertices)
    nv, dev = vertices.shape[0], vertices.device
    adj = _filter_adjacency('smooth', faces, nv, adjacency, dev)
    pin = _pinned('smooth', pinned, nv, dev, adj.boundary if pin_boundary else None)
    if iterations == 0 or nv == 0:
        return vertices.clone()
    return _smooth_steps(vertices, adj, pin, ([lam] if mu == 0.0 else [lam, mu]) * iterations)


def smooth_values(values, faces, iterations=1, factor=0.5, pinned=None, adjacency=None):
    """Laplacian smoothing of a per-vertex attribute [V, C], 1 <= C <= 256: ``iterations`` steps x <- x + factor (mean of the
    neighbours - x).  float32 values come back as float32; uint8 colours are smoothed as float32 and come back as
    floor(x + 0.5) clamped to uint8.  ``pinned`` and ``adjacency`` as for ``smooth``; nothing is pinned unless asked."""
    iterations = _iterations('smooth_values', iterations)
    factor = float(factor)
    if not math.isfinite(factor):
        raise ValueError(f'smooth_values: factor must be finite, got {factor}')
    values = torch.as_tensor(values).detach()
    if values.dtype not in (torch.float32, torch.uint8) or values.ndim != 2 or not 1 <= values.shape[1] <= 256 or values.shape[0] >= 2 ** 31 - 1:
        raise ValueError(f'smooth_values: values must be float32 or uint8 [V, C] with 1 <= C <= 256, got {values.dtype} {tuple(values.shape)}')
    nv, dev = values.shape[0], values.device
    adj = _filter_adjacency('smooth_values', faces, nv, adjacency, dev)
    pin = _pinned('smooth_values', pinned, nv, dev)
    x = values.to(torch.float32).contiguous()
    x = _smooth_steps(x, adj, pin, [factor] * iterations) if nv else x
    if values.dtype == torch.uint8:
        return torch.floor(x + 0.5).clamp(0, 255).to(torch.uint8)
    return x.clone() if iterations == 0 or nv == 0 else x


def _label_vote_cpu(labels, adj, pinned, n_labels):
    """p3d_mesh_label_vote's rule on uint8 labels: the counts of the neighbours' labels and the vertex's own, the smallest label
    that reaches the maximum unless the vertex's own does."""
    nv = labels.shape[0]
    counts = adj.offsets[1:] - adj.offsets[:-1]
    own = labels.long()
    source = torch.repeat_interleave(torch.arange(nv), counts)
    tally = torch.zeros([nv * n_labels], dtype=torch.int64)
    tally.index_add_(0, source * n_labels + own[adj.neighbours.long()], torch.ones_like(source))
    tally.index_add_(0, torch.arange(nv) * n_labels + own, torch.ones([nv], dtype=torch.int64))
    tally = tally.view(nv, n_labels)
    most = tally.max(1).values
    reaches = tally == most[:, None]
    smallest = torch.where(reaches, torch.arange(n_labels), torch.tensor(n_labels)).min(1).values
    new = torch.where(reaches.gather(1, own[:, None])[:, 0], own, smallest)
    moves = counts > 0
    if pinned is not None:
        moves &= pinned == 0
    return torch.where(moves, new, own).to(torch.uint8)


def smooth_labels(labels, faces, iterations=1, n_labels=None, pinned=None, adjacency=None):
    """Majority voting of per-vertex class labels (what removes the speckle an argmax leaves at part boundaries): int64 [V] on the
    labels' device.  Every iteration is one synchronous step: a vertex counts the labels of its neighbours and its own, keeps its
    label when that reaches the maximum count and otherwise takes the smallest label that does.  ``n_labels`` <= 256 (default: the
    largest label + 1); a label outside [0, n_labels) is a ValueError.  ``pinned`` and ``adjacency`` as for ``smooth``; vertices
    without neighbours keep their label.  Device labels run p3d_mesh_label_vote, one launch per step; CPU labels the same integer
    rule."""
    iterations = _iterations('smooth_labels', iterations)
    labels = torch.as_tensor(labels).detach()
    if labels.ndim != 1 or labels.dtype not in (torch.uint8, torch.int16, torch.int32, torch.int64) or labels.shape[0] >= 2 ** 31 - 1:
        raise ValueError(f'smooth_labels: labels must be an integer tensor [V], got {labels.dtype} {tuple(labels.shape)}')
    nv, dev = labels.shape[0], labels.device
    lo, hi = torch.stack(torch.aminmax(labels)).tolist() if nv else (0, 0)  # (on a device: one device-to-host copy)
    n_labels = hi + 1 if n_labels is None else int(n_labels)
    if not 1 <= n_labels <= 256:
        raise ValueError(f'smooth_labels: n_labels must be in [1, 256], got {n_labels}')
    if lo < 0 or hi >= n_labels:
        raise ValueError(f'smooth_labels: label outside [0, {n_labels}) (labels span [{lo}, {hi}])')
    adj = _filter_adjacency('smooth_labels', faces, nv, adjacency, dev)
    pin = _pinned('smooth_labels', pinned, nv, dev)
    x = labels.to(torch.uint8).contiguous()
    if nv == 0:
        return x.long()
    if not x.is_cuda:
        for _ in range(iterations):
            x = _label_vote_cpu(x, adj, pin, n_labels)
        return x.long()
    lib = _lib.lib()
    spare = [torch.empty_like(x), torch.empty_like(x)]
    for k in range(iterations):
        out = spare[k % 2]
        _lib.check(lib.p3d_mesh_label_vote(_lib.ptr(x), nv, n_labels, _lib.ptr(adj.offsets), _lib.ptr(adj.neighbours),
                                           adj.neighbours.shape[0], _lib.ptr(pin), _lib.ptr(out), _lib.stream_of(x)), 'mesh_label_vote')
        x = out
    return x.long()


# ---- labels and the whole script ---------------------------------------------------------------------------------------------
def default_palette(n):
    """uint8 [n, 3]: class 0 grey, the others spread round the hue circle by the golden angle (this package's own colours)."""
    import colorsys
    out = [(128, 128, 128)]
    for k in range(1, n):
        r, g, b = colorsys.hsv_to_rgb((k * 0.618033988749895) % 1.0, 0.65, 0.95)
        out.append((round(r * 255), round(g * 255), round(b * 255)))
    return torch.tensor(out[:n], dtype=torch.uint8)


@torch.no_grad()
def vertex_labels(G, ws, vertices, palette=None, max_batch=10_000_000):
    """extract_mesh.py:196-218: the argmax over G's semantic channels of G.sample_mixed at the vertices (in chunks of max_batch
    points), and its colour in ``palette`` uint8 [C, 3] (default: default_palette(C)).  Returns (labels int64 [V], colors uint8 [V, 3])
    on the vertices' device."""
    n_sem = int(G.semantic_channels)
    pts = vertices.detach().to(device=ws.device, dtype=torch.float32)[None]
    labels = torch.empty([pts.shape[1]], dtype=torch.int64, device=ws.device)
    for head in range(0, pts.shape[1], max_batch):
        out = G.sample_mixed(pts[:, head:head + max_batch], None, ws, truncation_psi=1, noise_mode='const')
        labels[head:head + max_batch] = out['rgb'][0, :, 32:32 + n_sem].argmax(dim=-1)
    pal = default_palette(n_sem) if palette is None else torch.as_tensor(palette, dtype=torch.uint8)
    return labels.to(vertices.device), pal.to(vertices.device)[labels.to(vertices.device)]


def _clean_geometry(G, ws, resolution, threshold, keep, min_faces, cell, tolerance=None, target_faces=None, **synthesis_kwargs):
    """extract_mesh's geometry: shape.extract_geometry and the optional clean-up (see ``extract_mesh``).  ``tolerance`` (world units)
    decimates through ``simplify_to`` instead of a given ``cell``, ``target_faces`` through ``decimate.decimate``; the three exclude
    each other."""
    if cell is not None and tolerance is not None:
        raise ValueError('cell= and tolerance= exclude each other: give the cell, or the tolerance that picks it')
    if target_faces is not None and (cell is not None or tolerance is not None):
        raise ValueError('target_faces= excludes cell= and tolerance=: quadric-error decimation to a face count, or vertex clustering')
    vertices, faces = shape.extract_geometry(G, ws, resolution, threshold, **synthesis_kwargs)
    if keep is not None or min_faces > 1:
        vertices, faces, _ = clean(vertices, faces, keep, min_faces)
    if target_faces is not None:
        from . import decimate                                             # (decimate imports this module)
        return decimate.decimate(vertices, faces, target_faces)[:2]        # collapses detach nothing: ``keep`` is not applied again
    if tolerance is not None and len(faces):
        vertices, faces, cell, _ = simplify_to(vertices, faces, tolerance)
    elif cell is not None:
        vertices, faces = simplify(vertices, faces, cell)
    if cell is not None:
        if keep is not None:
            vertices, faces, _ = clean(vertices, faces, keep)
    return vertices, faces


def _taubin(vertices, faces, iterations, lam, mu, adj):
    """``smooth`` for ``extract_mesh``, whose arguments ``smooth`` and ``smooth_labels`` hide the functions of those names."""
    return smooth(vertices, faces, iterations, lam, mu, adjacency=adj)


def _voted_colors(labels, faces, iterations, n_labels, palette, adj):
    """The palette colours (as ``vertex_labels`` picks them) of the labels after ``iterations`` voting steps."""
    labels = smooth_labels(labels, faces, iterations, n_labels, adjacency=adj)
    pal = default_palette(n_labels) if palette is None else torch.as_tensor(palette, dtype=torch.uint8)
    return pal.to(labels.device)[labels]


def script_turntable(G, n_frames=120):
    """(poses [n_frames, 4, 4], camera): the script's turntable for G, orthographic xmag = ymag = 0.3 at radius 1 about
    G.rendering_kwargs['avg_camera_pivot'] (an edge-map generator, the script's edge2car branch: 0.6 at 1.2, the full orbit)."""
    pivot = G.rendering_kwargs['avg_camera_pivot']
    if getattr(G, 'data_type', None) != 'edge':
        return turntable_poses(pivot, 1.0, n_frames), Orthographic(0.3, 0.3)
    poses = turntable_poses(pivot, 1.2, n_frames, yaw0=-_SCRIPT_PI / 2, yaw_range=np.pi, pitch_range=np.pi / 2)
    return poses, Orthographic(0.6, 0.6)


@torch.no_grad()
def extract_mesh(G, ws, resolution=512, threshold=50., n_frames=120, image_size=512, palette=None, keep=None, min_faces=1, cell=None,
                 smooth=0, smooth_labels=0, smooth_shading=False, lam=0.5, mu=-0.53, tolerance=None, target_faces=None, **synthesis_kwargs):
    """applications/extract_mesh.py after its inputs: shape.extract_geometry, per-vertex label colours unless G is an edge-map
    generator (data_type 'edge') or has no label channels, and the script's turntable — orthographic xmag = ymag = 0.3 at radius 1 (edge2car: 0.6 at 1.2) about
    G.rendering_kwargs['avg_camera_pivot'], image_size^2 pixels.  Returns (vertices, faces, vertex_colors or None, frames uint8
    [n_frames, image_size, image_size, 3]).  Clean-up, off by default, runs on the bare geometry before the labels and the
    turntable: ``clean(keep, min_faces)`` when ``keep`` is given or ``min_faces`` exceeds 1, then ``simplify(cell)`` when ``cell``
    (world units) is given, or ``simplify_to(tolerance)`` when ``tolerance`` (world units: the sampled Hausdorff distance the
    decimation may cost) is given instead, or ``decimate.decimate(target_faces)`` (quadric-error edge collapses down to that many faces, which keep ridges and necks and detach nothing) when ``target_faces`` is; any two together are a ValueError.  Clustering can pinch a thin neck into an edge, which no face carries, and so detach a crumb (and leaves
    the vertices of cells whose faces all collapsed): with both ``keep`` and ``cell`` the component count asked for is applied to the
    simplified mesh once more, so that keep=1 hands over one component.  Filtering, off by default too, follows the clean-up and
    leaves the faces alone: the labels are read at the unsmoothed vertices (the decoder's own level set), ``smooth_labels`` voting
    steps (``mesh.smooth_labels``) go over them before they become colours, ``smooth`` Taubin iterations with ``lam`` and ``mu``
    (``mesh.smooth``, boundary pinned) then move the vertices that are returned and rendered, and ``smooth_shading`` renders with
    ``texture.vertex_normals`` of that mesh instead of face normals."""
    vertices, faces = _clean_geometry(G, ws, resolution, threshold, keep, min_faces, cell, tolerance, target_faces, **synthesis_kwargs)
    edge = getattr(G, 'data_type', None) == 'edge'                      # the script's edge2car branch; every other generator is seg-like
    labelled = not edge and int(getattr(G, 'semantic_channels', 0) or 0) > 1
    adj = adjacency(faces, len(vertices)) if (smooth or smooth_labels) and len(vertices) else None
    colors = None
    if labelled and len(vertices):
        labels, colors = vertex_labels(G, ws, vertices, palette)
        if smooth_labels:
            colors = _voted_colors(labels, faces, smooth_labels, int(G.semantic_channels), palette, adj)
    if smooth and len(vertices):
        vertices = _taubin(vertices, faces, smooth, lam, mu, adj)
    shading = {}
    if smooth_shading and len(vertices):
        from . import texture                                              # (texture imports this module)
        shading['normals'] = texture.vertex_normals(vertices, faces)
    poses, camera = script_turntable(G, n_frames)
    frames = render(vertices, faces, poses, camera, image_size, colors=colors, **shading)
    return vertices, faces, colors, frames
