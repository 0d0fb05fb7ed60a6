"""Texture atlases for extracted meshes: a per-triangle UV layout, a texture image baked from rendered views, a renderer that samples
it, and OBJ + MTL + PNG export.

``texture.bake_colors`` keeps one colour per vertex, so appearance lives at the mesh's own resolution and is lost when the mesh is
decimated.  A texture image keeps it apart from the triangle count:

    v, f, layout, tex, seen, frames = atlas.atlas_mesh(G, ws, 'seg2cat', size=2048, cell=1 / 128, keep=1, path='cat.obj')

Every face gets half of a square cell of the image (``layout``); marching-cubes triangles are all bounded by one lattice cell, so a
uniform cell wastes little to size variance, and the layout is deterministic and integer-defined.  Decimate first (``cell=``): the
share of the image that carries colour falls with the cell (0.67 at cells of 9 texels, 0.29 at 4), and 400k faces leave a 2048^2 atlas
cells of 4.  Chart-based unwrapping, mip maps and inpainting of unseen texels are out of scope.

* ``layout`` / ``orient_faces`` / ``face_uv``: the atlas of T faces in a size^2 image, the corner order that puts a face's longest edge
  on the UV hypotenuse, and the UV coordinates of every corner.
* ``texel_points``: position, normal and face of every texel (p3d_mesh_atlas_texels).
* ``bake_texture``: the texels are points with normals, so the bake is ``texture.bake_accumulate`` / ``bake_finish`` on them against the
  mesh's raster buffers; ``assemble`` puts the colours into the image (p3d_mesh_atlas_assemble).
* ``shade_textured`` / ``render_textured``: ``mesh.shade`` / ``mesh.render`` with the albedo looked up in the texture
  (p3d_mesh_shade_textured): the operands and the CPU frame loop of ``mesh.shade``, the loop over groups of views of ``mesh.render``.
* ``write_obj``; ``atlas_views`` / ``atlas_mesh``: the generator's views baked into a texture, and the whole pipeline.

Device tensors run csrc/mesh_atlas.hip, CPU tensors the formulation below, written operation by operation: it is the definition
(include/p3d_hip.h, "mesh atlas"), and the kernels' bytes equal it.
"""
import math
import os
from typing import NamedTuple

import torch

from . import _lib, mesh, texture

GREY = mesh.GREY
MIN_SIZE, MAX_SIZE, MIN_CELL = 16, 8192, 4


# ---- layout -----------------------------------------------------------------------------------------------------------------
class AtlasLayout(NamedTuple):
    """``size`` x ``size`` texels in cells of ``cell`` x ``cell``, ``per_row`` cells per row; cell k holds faces 2 k and 2 k + 1."""
    size: int
    cell: int
    per_row: int
    n_faces: int

    @property
    def n_cells(self):
        return (self.n_faces + 1) // 2

    @property
    def side(self):
        """m: the side of a face's UV triangle, in texels."""
        return self.cell - 3

    @property
    def n_texels(self):
        """K: the texels of all used cells, in cell-major order."""
        return self.n_cells * self.cell * self.cell


def layout(n_faces, size):
    """The atlas of ``n_faces`` faces in a ``size`` x ``size`` image (16 <= size <= 8192): the largest ``cell`` for which the
    (size // cell)^2 cells hold the (n_faces + 1) // 2 pairs of faces.  A cell below 4 texels has no room for a triangle and its
    gutter: ValueError, naming the smallest size that would do."""
    if int(n_faces) != n_faces or int(size) != size:
        raise ValueError(f'layout: n_faces and size must be integers, got {n_faces!r}, {size!r}')
    n_faces, size = int(n_faces), int(size)
    if not 0 <= n_faces < 2 ** 31 - 1:
        raise ValueError(f'layout: n_faces must be in [0, 2^31 - 1), got {n_faces}')
    if not MIN_SIZE <= size <= MAX_SIZE:
        raise ValueError(f'layout: size must be in [{MIN_SIZE}, {MAX_SIZE}], got {size}')
    n_cells = (n_faces + 1) // 2
    across = math.isqrt(n_cells - 1) + 1 if n_cells else 1               # the fewest cells per row whose square holds n_cells
    cell = size // across
    if cell < MIN_CELL:
        raise ValueError(f'layout: {n_faces} faces leave a {size}^2 atlas cells of {cell} texels, below {MIN_CELL}: the smallest size '
                         f'that holds them is {MIN_CELL * across}' + (' (decimate the mesh first)' if MIN_CELL * across > MAX_SIZE else ''))
    return AtlasLayout(size, cell, size // cell, n_faces)


def _layout(what, lay, n_faces):
    """``lay`` (an AtlasLayout or a size) as the checked layout of ``n_faces`` faces."""
    if not isinstance(lay, AtlasLayout):
        return layout(n_faces, lay)
    if lay != layout(lay.n_faces, lay.size) or lay.n_faces != n_faces:
        raise ValueError(f'{what}: {lay} is not the layout of {n_faces} faces (atlas.layout({n_faces}, {lay.size}))')
    return lay


def _cell_grid(lay, device):
    """Per texel of the cell-major order: (cell index k, column i, row j), int64 [K] each."""
    q = torch.arange(lay.n_texels, dtype=torch.int64, device=device)
    cc = lay.cell * lay.cell
    k = torch.div(q, cc, rounding_mode='floor')
    rem = q - k * cc
    j = torch.div(rem, lay.cell, rounding_mode='floor')
    return k, rem - j * lay.cell, j


def texel_numerators(lay, device='cpu'):
    """(half, n0, n1, n2) int64 [K]: which face of its cell every texel belongs to (0 lower, 1 upper) and its barycentric numerators
    over ``lay.side``; n0 < 0 marks the gutter."""
    _, i, j = _cell_grid(lay, device)
    half = (i + j > lay.cell - 2).long()
    ip = torch.where(half == 1, lay.cell - 1 - i, i)
    jp = torch.where(half == 1, lay.cell - 1 - j, j)
    return half, lay.side - ip - jp, ip, jp


def face_uv(lay):
    """float32 [T, 3, 2]: (u, v) of every face's corners in the OBJ convention (origin bottom left, image row 0 at the top):
    u = (x + 0.5) / size, v = 1 - (y + 0.5) / size with (x, y) the texel whose centre the corner sits on."""
    t = torch.arange(lay.n_faces, dtype=torch.int64)
    k, upper = t >> 1, (t & 1) == 1
    m, top = lay.side, lay.cell - 1
    lower_xy = torch.tensor([[0, 0], [m, 0], [0, m]])
    upper_xy = torch.tensor([[top, top], [top - m, top], [top, top - m]])
    xy = torch.where(upper[:, None, None], upper_xy, lower_xy)            # [T, 3, 2]
    x = (k % lay.per_row * lay.cell)[:, None] + xy[..., 0]
    y = (torch.div(k, lay.per_row, rounding_mode='floor') * lay.cell)[:, None] + xy[..., 1]
    return torch.stack([(x.double() + 0.5) / lay.size, 1.0 - (y.double() + 0.5) / lay.size], dim=-1).float()


# ---- corner order -----------------------------------------------------------------------------------------------------------
def orient_faces(vertices, faces):
    """faces int64 [T, 3] with every face's corners rotated (cyclically: the winding stays) so that its longest edge lies opposite
    corner 0 and becomes the UV hypotenuse, which stretches the texture least.  Squared lengths in fp64, (dx dx + dy dy) + dz dz; ties
    go to the lowest corner, so oriented faces stay as they are.  Torch operations on the vertices' device; the same on every device.
    Everything downstream takes these as THE faces: the file, the rasterizer, the atlas."""
    vertices = mesh._mesh_vertices('orient_faces', vertices)
    faces = mesh._mesh_faces('orient_faces', faces, vertices.shape[0]).to(vertices.device)
    p = vertices.double()[faces]                                          # [T, 3, 3]

    def length(a, b):
        d = p[:, b] - p[:, a]
        s = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        return s + d[:, 2] * d[:, 2]
    l0, l1, l2 = length(1, 2), length(2, 0), length(0, 1)                 # the edge opposite corner 0, 1, 2
    first = torch.where((l0 >= l1) & (l0 >= l2), 0, torch.where(l1 >= l2, 1, 2))
    order = (first[:, None] + torch.arange(3, device=faces.device)) % 3
    return faces.gather(1, order)


# ---- texel geometry ---------------------------------------------------------------------------------------------------------
def _texels_cpu(vertices, faces, normals, lay):
    k, _, _ = _cell_grid(lay, 'cpu')
    half, n0, n1, n2 = texel_numerators(lay)
    t = 2 * k + half
    nv = vertices.shape[0]
    ok = t < lay.n_faces
    idx = faces.long()[t.clamp(max=max(lay.n_faces - 1, 0))]              # [K, 3]
    ok &= ((idx >= 0) & (idx < nv)).all(1)
    idx = idx.clamp(0, max(nv - 1, 0))
    n0, n1, n2, m = n0.double()[:, None], n1.double()[:, None], n2.double()[:, None], float(lay.side)
    out = []
    for field in (vertices, normals):
        a = field.double()
        s = n0 * a[idx[:, 0]]
        s = s + n1 * a[idx[:, 1]]
        s = s + n2 * a[idx[:, 2]]
        out.append(torch.where(ok[:, None], s / m, torch.zeros_like(s)).float())
    return out[0], out[1], torch.where(ok, t, torch.full_like(t, -1)).to(torch.int32)


def texel_points(vertices, faces, normals, lay):
    """(points float32 [K, 3], texel_normals float32 [K, 3], face int32 [K]) of the atlas's texels in cell-major order
    (q = (k cell + j) cell + i): the face a texel belongs to, and the mix (n0 a0 + n1 a1 + n2 a2) / side of the face's corner positions
    and vertex normals — linear extrapolation in the gutter, the vertex itself, bit for bit, at a corner.  The normals are not
    normalised.  face is -1, with a zero point and normal, where the face does not exist (the upper half of the last cell for an odd
    number of faces) or has a vertex index outside [0, V)."""
    vertices = mesh._mesh_vertices('texel_points', vertices)
    nv, dev = vertices.shape[0], vertices.device
    faces32 = mesh._faces32(faces).to(dev)
    lay = _layout('texel_points', lay, faces32.shape[0])
    normals = texture._normals('texel_points', normals, vertices)
    if not vertices.is_cuda:
        return _texels_cpu(vertices, faces32, normals, lay)
    k = lay.n_texels
    points, tnormals = torch.empty([k, 3], dtype=torch.float32, device=dev), torch.empty([k, 3], dtype=torch.float32, device=dev)
    face = torch.empty([k], dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().p3d_mesh_atlas_texels(_lib.ptr(vertices), nv, _lib.ptr(faces32), lay.n_faces, _lib.ptr(normals), lay.size, lay.cell,
                                                _lib.ptr(points), _lib.ptr(tnormals), _lib.ptr(face), _lib.stream_of(vertices)),
               'mesh_atlas_texels')
    return points, tnormals, face


# ---- the image --------------------------------------------------------------------------------------------------------------
def _rgb(what, value):
    rgb = tuple(int(x) for x in value)
    if len(rgb) != 3 or not all(0 <= x <= 255 for x in rgb):
        raise ValueError(f'{what} must be three values in 0 .. 255, got {value!r}')
    return rgb


def assemble(colors, face, lay, background=(GREY, GREY, GREY)):
    """The texture uint8 [size, size, 3] from the texels' colours uint8 [K, 3] and faces int32 [K] (``texel_points``): texel (i, j) of
    cell k at row (k // per_row) cell + j, column (k % per_row) cell + i; ``background`` for texels without a face, unused cells and
    the margins right of and below the cells."""
    if not isinstance(lay, AtlasLayout):
        raise TypeError(f'assemble: lay must be an AtlasLayout, got {type(lay).__name__}')
    lay = _layout('assemble', lay, lay.n_faces)
    bg = _rgb('assemble: background', background)
    k, dev = lay.n_texels, colors.device
    if colors.dtype != torch.uint8 or tuple(colors.shape) != (k, 3) or tuple(face.shape) != (k,):
        raise ValueError(f'assemble: colors must be uint8 [{k}, 3] and face [{k}], got {colors.dtype} {tuple(colors.shape)} and '
                         f'{tuple(face.shape)}')
    colors = colors.detach().contiguous()
    face = face.detach().to(device=dev, dtype=torch.int32).contiguous()
    if not colors.is_cuda:
        out = torch.empty([lay.size, lay.size, 3], dtype=torch.uint8)
        out[:] = torch.tensor(bg, dtype=torch.uint8)
        ck, i, j = _cell_grid(lay, 'cpu')
        row = torch.div(ck, lay.per_row, rounding_mode='floor') * lay.cell + j
        col = ck % lay.per_row * lay.cell + i
        out[row, col] = torch.where((face >= 0)[:, None], colors, out[row, col])
        return out
    out = torch.empty([lay.size, lay.size, 3], dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().p3d_mesh_atlas_assemble(_lib.ptr(colors), _lib.ptr(face), lay.n_faces, lay.size, lay.cell, *bg, _lib.ptr(out),
                                                  _lib.stream_of(out)), 'mesh_atlas_assemble')
    return out


# ---- baking -----------------------------------------------------------------------------------------------------------------
def _bake(what, vertices, faces32, texels, lay, images, c2w, camera, tolerance, power, min_cos, fallback, background, max_bytes):
    points, tnormals, face = texels
    dev, size = vertices.device, tuple(images.shape[1:3])
    nk = lay.n_texels
    images = images.detach().to(dev).contiguous()
    acc, seen = texture.bake_buffers(nk, dev)
    for part, poses, cam in mesh._view_groups(what, c2w, camera, nk, max_bytes) if nk else ():
        proj, face_id, depth = mesh._raster_group(vertices, faces32, poses, cam, size)
        del proj                                                           # before the texels' is made: max_bytes bounds what is alive at once
        proj = mesh.project(points, poses, cam, size)
        texture.bake_accumulate(acc, seen, proj, face_id, depth, images[part], points, tnormals, poses, tolerance, power, min_cos)
        del proj, face_id, depth
    colors = texture.bake_finish(acc, fallback)
    seen = torch.where(face >= 0, seen, torch.zeros_like(seen))          # (at min_cos = 0 the zero normal of a texel without a face counts)
    return assemble(colors, face, lay, background), seen


def _bake_mesh(what, vertices, faces, normals, lay):
    vertices = mesh._mesh_vertices(what, vertices)
    faces32 = mesh._mesh_faces(what, faces, vertices.shape[0]).to(device=vertices.device, dtype=torch.int32)
    lay = _layout(what, lay, faces32.shape[0])
    return vertices, faces32, texture._normals(what, normals, vertices, faces32), lay


@torch.no_grad()
def bake_texture(vertices, faces, images, cam2world, camera, layout_or_size, normals=None, tolerance=0.01, power=2, min_cos=0.1,
                 fallback=(GREY, GREY, GREY), background=(GREY, GREY, GREY), max_bytes=1 << 30):
    """(texture uint8 [size, size, 3], seen int32 [K]) of the mesh (vertices float32 [V, 3], faces [T, 3], as ``orient_faces`` left
    them) from ``images`` uint8 [F, H, W, 3], frames of the cameras ``cam2world`` [F, 4, 4] / ``camera``: ``texture.bake_colors`` with
    the K texels of the atlas (``layout_or_size``: an ``AtlasLayout`` or the image's size) in the place of the vertices.  Every texel
    is a point with a normal (``texel_points``; ``normals`` default to ``texture.vertex_normals``), projected like a vertex and tested
    against the MESH's raster buffers, and takes the cos^power-weighted mean of the frames that see it; a texel no frame sees takes
    ``fallback`` (uint8 [K, 3] or one RGB triple), and what is no texel of a face takes ``background``.  ``seen`` counts the frames per
    texel, in cell-major order.  ``tolerance`` .. ``min_cos`` as for ``bake_colors``.  The views go through project / rasterize /
    accumulate in groups of at most ``max_bytes`` of projected texels (16 K bytes per view); the result does not depend on the
    grouping.  Everything runs on the vertices' device."""
    texture._bake_parameters(tolerance, power, min_cos)
    vertices, faces32, normals, lay = _bake_mesh('bake_texture', vertices, faces, normals, layout_or_size)
    images, c2w, camera = texture._views('bake_texture', images, cam2world, camera)
    texture._fallback(fallback, lay.n_texels, vertices.device)             # checked here: before any launch
    _rgb('bake_texture: background', background)
    texels = texel_points(vertices, faces32, normals, lay)
    return _bake('bake_texture', vertices, faces32, texels, lay, images, c2w, camera, tolerance, power, min_cos, fallback, background,
                 max_bytes)


# ---- rendering with the texture ---------------------------------------------------------------------------------------------
def _lookup(b1, b2, t, lay):
    """The bilinear lookup of include/p3d_hip.h for barycentrics b1, b2 (fp64, in the stored corner order) on faces t: the first tap's
    (row, column) in the image and the weights fx, fy in 1 / 256."""
    cell, top, m = lay.cell, lay.cell - 1, float(lay.side)
    upper = (t & 1) == 1
    x, y = b1 * m, b2 * m
    x, y = torch.where(upper, float(top) - x, x), torch.where(upper, float(top) - y, y)

    def fixed(v):
        v = torch.round(v * 256.0)                                         # half to even
        return torch.where(v >= 0, v.clamp(max=float(top * 256)), torch.zeros_like(v)).long()       # (NaN -> 0)
    xi, yi = fixed(x), fixed(y)
    c0, r0 = (xi >> 8).clamp(max=cell - 2), (yi >> 8).clamp(max=cell - 2)
    k = t >> 1
    row = torch.div(k, lay.per_row, rounding_mode='floor') * cell + r0
    col = k % lay.per_row * cell + c0
    return row, col, xi - (c0 << 8), yi - (r0 << 8)


def _atlas_albedo(faces, tex, lay):
    """The albedo of ``shade_textured`` for ``mesh._shade_cpu``: the lookup and the integer bilinear mix of the 2 x 2 texels."""
    tex = tex.long()

    def albedo(t, idx, b):
        swapped = idx[:, 1] != faces[t, 1].long()                          # back into the stored corner order
        row, col, fx, fy = _lookup(torch.where(swapped, b[2], b[1]), torch.where(swapped, b[1], b[2]), t, lay)
        num = (256 - fy)[:, None] * ((256 - fx)[:, None] * tex[row, col] + fx[:, None] * tex[row, col + 1]) + \
            fy[:, None] * ((256 - fx)[:, None] * tex[row + 1, col] + fx[:, None] * tex[row + 1, col + 1])      # exact integers
        return num.double() / 65536.0
    return albedo


def shade_textured(face_id, proj, vertices, faces, cam2world, tex, lay, background=(255, 255, 255), ambient=0.3):
    """``mesh.shade`` with the albedo looked up in the texture ``tex`` uint8 [size, size, 3] of the atlas ``lay`` of these faces: the
    pixel's barycentrics, in the face's stored corner order, give a point of the face's UV triangle, and the albedo is the bilinear mix
    of the 2 x 2 texels around it with weights in 1 / 256 (include/p3d_hip.h).  Every input is moved to face_id's device, which picks
    the path."""
    face_id, proj, vertices, faces32, cams, bg = mesh._shade_operands('shade_textured', face_id, proj, vertices, faces, cam2world, background)
    lay = _layout('shade_textured', lay, faces32.shape[0])
    tex = torch.as_tensor(tex)
    if tex.dtype != torch.uint8 or tuple(tex.shape) != (lay.size, lay.size, 3):
        raise ValueError(f'shade_textured: the texture must be uint8 [{lay.size}, {lay.size}, 3], got {tex.dtype} {tuple(tex.shape)}')
    tex = tex.detach().to(face_id.device).contiguous()
    if not face_id.is_cuda:
        return mesh._shade_cpu(face_id, proj, vertices, faces32, cams, ambient, bg, _atlas_albedo(faces32, tex, lay))
    n, h, w = face_id.shape
    rgb = torch.empty([n, h, w, 3], dtype=torch.uint8, device=face_id.device)
    _lib.check(_lib.lib().p3d_mesh_shade_textured(_lib.ptr(face_id), _lib.ptr(proj.packed), _lib.ptr(vertices), vertices.shape[0],
                                                  _lib.ptr(faces32), lay.n_faces, _lib.ptr(tex), lay.size, lay.cell, _lib.ptr(cams), n,
                                                  int(proj.orthographic), w, h, float(ambient), *bg, _lib.ptr(rgb), _lib.stream_of(rgb)),
               'mesh_shade_textured')
    return rgb


@torch.no_grad()
def render_textured(vertices, faces, cam2world, camera, resolution, tex, lay, background=(255, 255, 255), ambient=0.3, return_buffers=False,
                    max_bytes=1 << 30):
    """``mesh.render`` with ``shade_textured`` as its last stage: uint8 frames [F, H, W, 3] of the mesh with the texture ``tex`` of the
    atlas ``lay``, on the vertices' device; with return_buffers=True also (face_id, depth)."""
    size = mesh._size(resolution)
    faces32 = mesh._faces32(faces)                                         # checked before the layout; _render takes them as they are (no second copy)
    lay = _layout('render_textured', lay, faces32.shape[0])
    tex = torch.as_tensor(tex).to(vertices.device)

    def stage(*buffers):
        return shade_textured(*buffers, tex, lay, background, ambient)
    return mesh._render('render_textured', vertices, faces32, cam2world, camera, size, stage, return_buffers, max_bytes)


# ---- files ------------------------------------------------------------------------------------------------------------------
def write_obj(path, vertices, faces, lay, tex, normals=None):
    """Wavefront OBJ with its material and image: ``path`` (.obj: ``v``, optional ``vn``, three ``vt`` per face from ``face_uv``,
    ``f a/ta[/na]`` with 1-based indices, ``mtllib`` and ``usemtl atlas``), and beside it <name>.mtl (``newmtl atlas``, ``Kd 1 1 1``,
    ``map_Kd <name>.png``) and <name>.png, the texture, written through PIL."""
    from PIL import Image
    path = os.fspath(path)
    stem, ext = os.path.splitext(path)
    if ext.lower() != '.obj':
        raise ValueError(f'write_obj: the path must end in .obj, got {path!r}')
    v = vertices.detach().cpu().to(torch.float32)
    f = mesh._mesh_faces('write_obj', faces.detach().cpu(), len(v)).numpy()
    lay = _layout('write_obj', lay, len(f))
    tex = torch.as_tensor(tex).detach().cpu()
    if tex.dtype != torch.uint8 or tuple(tex.shape) != (lay.size, lay.size, 3):
        raise ValueError(f'write_obj: the texture must be uint8 [{lay.size}, {lay.size}, 3], got {tex.dtype} {tuple(tex.shape)}')
    name = os.path.basename(stem)
    lines = [f'mtllib {name}.mtl', 'usemtl atlas']
    lines += ['v %.9g %.9g %.9g' % tuple(p) for p in v.tolist()]
    if normals is not None:
        n = torch.as_tensor(normals).detach().cpu().to(torch.float32)
        if n.shape != v.shape:
            raise ValueError(f'write_obj: normals must be [V, 3] like the vertices, got {tuple(n.shape)}')
        lines += ['vn %.9g %.9g %.9g' % tuple(p) for p in n.tolist()]
    lines += ['vt %.9g %.9g' % tuple(p) for p in face_uv(lay).reshape(-1, 2).tolist()]
    corner = 'f %d/%d/%d %d/%d/%d %d/%d/%d' if normals is not None else 'f %d/%d %d/%d %d/%d'
    for t, (a, b, c) in enumerate((f + 1).tolist()):
        ids = ((a, 3 * t + 1), (b, 3 * t + 2), (c, 3 * t + 3))
        lines.append(corner % tuple(x for vi, ti in ids for x in ((vi, ti, vi) if normals is not None else (vi, ti))))
    with open(path, 'w', encoding='ascii') as fh:
        fh.write('\n'.join(lines) + '\n')
    with open(stem + '.mtl', 'w', encoding='ascii') as fh:
        fh.write(f'newmtl atlas\nKd 1 1 1\nmap_Kd {name}.png\n')
    Image.fromarray(tex.numpy()).save(stem + '.png')


# ---- the generator's views and the whole pipeline ---------------------------------------------------------------------------
@torch.no_grad()
def atlas_views(G, ws, vertices, faces, cfg='seg2cat', size=2048, n_views=24, jitter='frozen', return_frames=False, render_kwargs=None,
                normals=None, **bake_kwargs):
    """Bake ``n_views`` views of the latent ``ws`` into a texture: ``texture.bake_views`` with ``bake_texture`` in the place of
    ``bake_colors``.  The fallback, unless given, is the decoder's own colour at the texels (``texture.vertex_rgb`` of their points).
    Returns (texture uint8 [size, size, 3], seen int32 [K], layout), and with ``return_frames`` also the dict of ``render_views``."""
    params = dict(tolerance=0.01, power=2, min_cos=0.1, background=(GREY, GREY, GREY), max_bytes=1 << 30)
    unknown = set(bake_kwargs) - set(params) - {'fallback'}
    if unknown:
        raise TypeError(f'atlas_views: unexpected arguments {sorted(unknown)}')
    params.update({k: v for k, v in bake_kwargs.items() if k != 'fallback'})
    texture._bake_parameters(params['tolerance'], params['power'], params['min_cos'])
    _rgb('atlas_views: background', params['background'])
    vertices, faces32, normals, lay = _bake_mesh('atlas_views', vertices, faces, normals, size)
    if 'fallback' in bake_kwargs:
        texture._fallback(bake_kwargs['fallback'], lay.n_texels, vertices.device)
    frames, c2w, camera = texture._generator_views(G, ws, cfg, n_views, jitter, render_kwargs)
    images, c2w, camera = texture._views('atlas_views', frames['image'], c2w, camera)
    texels = texel_points(vertices, faces32, normals, lay)
    fallback = bake_kwargs['fallback'] if 'fallback' in bake_kwargs else texture.vertex_rgb(G, ws, texels[0])
    tex, seen = _bake('atlas_views', vertices, faces32, texels, lay, images, c2w, camera, fallback=fallback, **params)
    return (tex, seen, lay, frames) if return_frames else (tex, seen, lay)


@torch.no_grad()
def atlas_mesh(G, ws, cfg='seg2cat', size=2048, resolution=512, threshold=50., n_frames=120, image_size=512, keep=None, min_faces=1,
               cell=None, n_views=24, jitter='frozen', path=None, bake_kwargs=None, render_kwargs=None, smooth=0, tolerance=None, target_faces=None, **synthesis_kwargs):
    """``texture.textured_mesh`` with a texture image instead of vertex colours: the clean-up geometry of ``mesh.extract_mesh``
    (``resolution`` .. ``cell``, or ``tolerance`` or ``target_faces`` in its place; decimate with either so that the faces fit the atlas with cells worth having), ``orient_faces``,
    vertex normals, a ``size``^2 texture baked from ``n_views`` views (``atlas_views``; ``bake_kwargs`` go to the bake, ``render_kwargs``,
    on top of ``synthesis_kwargs``, to ``views.render_views``), the script's
    turntable rendered with it, and, with ``path``, the OBJ with its MTL and PNG.  ``smooth`` Taubin iterations (``mesh.smooth`` at its
    defaults) move the vertices right after the clean-up, before anything is oriented or baked.  Returns (vertices, faces, layout,
    texture uint8 [size, size, 3], seen int32 [K], frames uint8 [n_frames, image_size, image_size, 3])."""
    vertices, faces = mesh._clean_geometry(G, ws, resolution, threshold, keep, min_faces, cell, tolerance, target_faces, **synthesis_kwargs)
    if smooth and len(vertices):
        vertices = mesh.smooth(vertices, faces, smooth)
    faces = orient_faces(vertices, faces)
    lay = layout(faces.shape[0], size)                                     # too many faces for the size: said before anything is rendered
    normals = texture.vertex_normals(vertices, faces)
    tex, seen, lay = atlas_views(G, ws, vertices, faces, cfg, lay, n_views, jitter, render_kwargs=dict(synthesis_kwargs, **(render_kwargs or {})),
                                 normals=normals,
                                 **(bake_kwargs or {}))
    poses, camera = mesh.script_turntable(G, n_frames)
    frames = render_textured(vertices, faces, poses, camera, image_size, tex, lay)
    if path is not None:
        write_obj(path, vertices, faces, lay, tex, normals=normals)
    return vertices, faces, lay, tex, seen, frames
