"""Texture atlases (pix2pix3d_amd/atlas.py), CPU formulation: the layout, footprints that stay on their own face, texel geometry
against a per-texel loop, bakes of known colours, held-out views, occlusion, view groups, the textured shade against a per-pixel
loop, the OBJ, argument checks, a CPU generator."""
import ctypes
import math

import numpy as np
import pytest
import torch

from pix2pix3d_amd import atlas, mesh, texture
from test_mesh_host import check_view_groups, grouped_views
from test_texture_host import camera_kinds, fib_cameras, flat_frames, small_generator, sphere_scene, two_sphere_scene

_cache = {}


# ---- scenes shared with test_atlas_gpu.py ----------------------------------------------------------------------------------------
def oriented(name):
    """(vertices, oriented faces, true colours, vertex normals) of a scene of test_texture_host.py, computed once."""
    if name not in _cache:
        v, f, colors = sphere_scene() if name == 'sphere' else two_sphere_scene()
        f = atlas.orient_faces(v, f)
        _cache[name] = (v, f, colors, texture.vertex_normals(v, f))
    return _cache[name]


def scene_views(name, kind):
    """(poses, camera, frames in the true colours) of a scene: 14 views of 128^2 (sphere) or 96^2 (two spheres)."""
    if (name, kind) not in _cache:
        v, f, colors, _ = oriented(name)
        focal, size = (4.2647, 128) if name == 'sphere' else (2.2, 96)
        poses, cam = camera_kinds(focal)[kind]
        _cache[name, kind] = (poses, cam, flat_frames(v, f, colors, poses, cam, size))
    return _cache[name, kind]


def baked(name, kind, size):
    """(layout, texture, seen) of a scene's bake at the default parameters, computed once and left unchanged."""
    if (name, kind, size) not in _cache:
        v, f, _, n = oriented(name)
        poses, cam, frames = scene_views(name, kind)
        lay = atlas.layout(len(f), size)
        _cache[name, kind, size] = (lay,) + atlas.bake_texture(v, f, frames, poses, cam, lay, normals=n)
    return _cache[name, kind, size]


def texel_colours(tex, lay):
    """uint8 [K, 3]: the texture read back at every texel of the cell-major order."""
    k, i, j = atlas._cell_grid(lay, 'cpu')
    return tex[k // lay.per_row * lay.cell + j, k % lay.per_row * lay.cell + i]


def texel_truth(lay, f, colors, face):
    """The rounded barycentric mix of the true vertex colours at every texel (extrapolated in the gutter), and n0."""
    _, n0, n1, n2 = atlas.texel_numerators(lay)
    corner = colors.double()[f[face.long().clamp(min=0)]]                  # [K, 3, 3]
    mix = (n0[:, None] * corner[:, 0] + n1[:, None] * corner[:, 1] + n2[:, None] * corner[:, 2]) / lay.side
    return torch.round(mix), n0


# ---- 1. layout --------------------------------------------------------------------------------------------------------------------
def test_layout_takes_the_largest_cell_that_fits():
    for n_faces, size in [(1, 16), (2, 16), (3, 16), (7, 64), (13_856, 336), (13_856, 512), (3_704, 256), (100_000, 2048), (400_000, 4096),
                          (400_000, 2048), (33, 100), (513, 1000)]:
        lay = atlas.layout(n_faces, size)
        n_cells = (n_faces + 1) // 2
        assert lay.size == size and lay.n_faces == n_faces and lay.n_cells == n_cells and lay.per_row == size // lay.cell
        assert lay.cell >= 4 and (size // lay.cell) ** 2 >= n_cells
        assert lay.cell == size or (size // (lay.cell + 1)) ** 2 < n_cells, 'a larger cell would fit'
        assert lay.side == lay.cell - 3 and lay.n_texels == n_cells * lay.cell ** 2
    assert atlas.layout(1, 16).cell == 16 and atlas.layout(2, 16).cell == 16 and atlas.layout(3, 16).cell == 8
    assert atlas.layout(33, 100) == atlas.AtlasLayout(100, 20, 5, 33)        # 17 cells on 5 x 5
    assert atlas.layout(513, 1000) == atlas.AtlasLayout(1000, 58, 17, 513)   # 257 cells on 17 x 17 of 58: a margin of 14 texels
    assert atlas.layout(100_000, 2048).cell == 9 and atlas.layout(400_000, 4096).cell == 9 and atlas.layout(400_000, 2048).cell == 4
    assert atlas.layout(13_856, 336).cell == 4 and atlas.layout(13_856, 512).cell == 6 and atlas.layout(3_704, 256).cell == 5
    with pytest.raises(ValueError, match='smallest size that holds them is 336'):
        atlas.layout(13_856, 256)
    with pytest.raises(ValueError, match='smallest size that holds them is 336'):
        atlas.layout(13_856, 335)
    for bad in [(4, 15), (4, 8193), (-1, 64), (4, 64.5), (2 ** 31 - 1, 64)]:
        with pytest.raises(ValueError, match='layout'):
            atlas.layout(*bad)


def test_no_texel_of_the_two_sphere_atlas_is_owned_twice():
    v, f, _, n = oriented('two')
    assert len(f) == 3_704
    lay = atlas.layout(len(f), 256)
    assert lay.cell == 5
    _, _, face = atlas.texel_points(v, f, n, lay)
    ids = torch.arange(lay.n_texels, dtype=torch.int32)
    owner = atlas.assemble(torch.stack([ids & 255, (ids >> 8) & 255, ids >> 16], dim=1).to(torch.uint8), face, lay, background=(255, 255, 255))
    owner = owner[..., 0].int() | (owner[..., 1].int() << 8) | (owner[..., 2].int() << 16)
    placed = owner[owner != 0xffffff]
    assert len(placed) == lay.n_texels == len(placed.unique())                # every texel once, none twice
    count = torch.bincount(face.long(), minlength=len(f))
    assert torch.equal(count[0::2], torch.full([lay.n_cells], 10)) and torch.equal(count[1::2], torch.full([lay.n_cells], 15))


# ---- 2. footprints ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cell', [4, 5, 6, 9, 16])
def test_bilinear_footprints_stay_on_the_sampled_face(cell):
    """Every tap of the lookup rule with a non-zero weight lies on a texel whose ``face`` is the sampled face.  Measured: 0 stray taps
    for every cell and half (20 000 random points, the corners and the edge midpoints each)."""
    m = cell - 3
    v, f, _, n = oriented('two')
    lay = atlas.layout(32, 4 * cell)                                            # 16 cells of this size on a 4 x 4 grid
    assert lay.cell == cell
    face = atlas.texel_points(v, f[:32], n, lay)[2].reshape(16, cell, cell)[5]   # [j][i] of cell 5: faces 10 and 11
    g = torch.Generator().manual_seed(cell)
    r = torch.rand([20_000, 2], generator=g, dtype=torch.float64)
    flip = r.sum(1) > 1
    r = torch.where(flip[:, None], 1 - r, r)                                   # uniform over b1 + b2 <= 1
    special = torch.tensor([[0, 0], [1, 0], [0, 1], [0.5, 0], [0, 0.5], [0.5, 0.5]], dtype=torch.float64)
    b1, b2 = torch.cat([special, r]).unbind(1)
    for half in (0, 1):
        x, y = b1 * m, b2 * m
        if half:
            x, y = (cell - 1) - x, (cell - 1) - y
        X = torch.round(x * 256).clamp(0, (cell - 1) * 256).long()
        Y = torch.round(y * 256).clamp(0, (cell - 1) * 256).long()
        c0, r0 = (X >> 8).clamp(max=cell - 2), (Y >> 8).clamp(max=cell - 2)
        fx, fy = X - (c0 << 8), Y - (r0 << 8)
        assert int(fx.min()) >= 0 and int(fx.max()) <= 256 and int(fy.min()) >= 0 and int(fy.max()) <= 256
        stray = 0
        for dr, dc, wgt in ((0, 0, (256 - fy) * (256 - fx)), (0, 1, (256 - fy) * fx), (1, 0, fy * (256 - fx)), (1, 1, fy * fx)):
            i, j = c0 + dc, r0 + dr
            assert int(i.max()) <= cell - 1 and int(j.max()) <= cell - 1
            stray += int(((wgt != 0) & (face[j, i] != 10 + half)).sum())
        print(f'cell {cell} half {half}: {stray} stray taps')
        assert stray == 0


# ---- 3. texel geometry --------------------------------------------------------------------------------------------------------------
def loop_texels(vertices, faces, normals, lay):
    v, n, f = vertices.double().tolist(), normals.double().tolist(), faces.tolist()
    cell, m = lay.cell, lay.cell - 3
    pts, nrm, face = [], [], []
    for k in range(lay.n_cells):
        for j in range(cell):
            for i in range(cell):
                half = 1 if i + j > cell - 2 else 0
                ip, jp = (cell - 1 - i, cell - 1 - j) if half else (i, j)
                num = (m - ip - jp, ip, jp)
                t = 2 * k + half
                if t >= len(f) or not all(0 <= c < len(v) for c in f[t]):
                    pts.append([0.0] * 3); nrm.append([0.0] * 3); face.append(-1)
                    continue
                face.append(t)
                for src, dst in ((v, pts), (n, nrm)):
                    a = [src[c] for c in f[t]]
                    dst.append([(float(num[0]) * a[0][d] + float(num[1]) * a[1][d] + float(num[2]) * a[2][d]) / float(m) for d in range(3)])
    return (torch.tensor(pts, dtype=torch.float64).float().reshape(-1, 3), torch.tensor(nrm, dtype=torch.float64).float().reshape(-1, 3),
            torch.tensor(face, dtype=torch.int32))


@pytest.mark.parametrize('n_faces,size', [(1, 16), (2, 16), (301, 100), (300, 64)])
def test_texel_points_equal_a_per_texel_loop(n_faces, size):
    v, f, _, n = oriented('two')
    f = f[:n_faces].clone()
    if n_faces == 300:
        f[17, 2] = len(v)                                                      # an index out of range: the face has no texels
    lay = atlas.layout(n_faces, size)
    pts, nrm, face = atlas.texel_points(v, f, n, lay)
    want = loop_texels(v, f, n, lay)
    assert pts.dtype == torch.float32 and nrm.dtype == torch.float32 and face.dtype == torch.int32 and tuple(pts.shape) == (lay.n_texels, 3)
    assert torch.equal(face, want[2]) and torch.equal(pts, want[0]) and torch.equal(nrm, want[1])
    assert (face == -1).any() == (n_faces in (1, 301, 300))
    if n_faces == 300:
        assert not (face == 17).any() and (face == 16).any()
    # a texel at a corner is the vertex, bit for bit
    cc, m, top = lay.cell ** 2, lay.side, lay.cell - 1
    for t in range(n_faces):
        if n_faces == 300 and t == 17:
            continue
        at = [(0, 0), (m, 0), (0, m)] if t % 2 == 0 else [(top, top), (top - m, top), (top, top - m)]
        for corner, (i, j) in enumerate(at):
            q = (t // 2) * cc + j * lay.cell + i
            assert int(face[q]) == t and torch.equal(pts[q], v[f[t, corner]]) and torch.equal(nrm[q], n[f[t, corner]])


def test_orient_faces_puts_the_longest_edge_opposite_corner_0():
    v, f, _ = sphere_scene()
    o = atlas.orient_faces(v, f)
    assert o.dtype == torch.int64 and o.shape == f.shape
    p = v.double()[o]
    l0 = (p[:, 2] - p[:, 1]).pow(2).sum(1)
    assert (l0 >= (p[:, 0] - p[:, 2]).pow(2).sum(1) - 1e-15).all() and (l0 >= (p[:, 1] - p[:, 0]).pow(2).sum(1) - 1e-15).all()
    # a cyclic rotation: the same corners in the same winding
    shift = (o[:, :1] == f).long().argmax(1)
    assert torch.equal(o, f.gather(1, (shift[:, None] + torch.arange(3)) % 3))
    assert len(shift.unique()) == 3                                            # all three rotations occur
    assert torch.equal(atlas.orient_faces(v, o), o)                            # oriented faces stay
    # ties go to the lowest corner: an equilateral face and an isosceles one with its two longest edges opposite corners 1 and 2
    tv = torch.tensor([[0.0, 0, 0], [3, 4, 0], [4, 3, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    tf = torch.tensor([[3, 4, 5], [0, 1, 2], [2, 0, 1]])
    assert atlas.orient_faces(tv, tf).tolist() == [[3, 4, 5], [1, 2, 0], [2, 0, 1]]


# ---- 4. the smooth sphere -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
def test_bake_of_the_smooth_sphere(kind):
    """Measured with this formulation, both camera kinds, size 512 (cell 6): every live texel seen; texels with n0 >= 0 off by at most
    1 level from the rounded mix of the true vertex colours (bound 2: one level of margin); gutter texels by 5, against an
    extrapolated "truth" nobody sees (not bounded here: the held-out views cover them)."""
    v, f, colors, n = oriented('sphere')
    lay, tex, seen = baked('sphere', kind, 512)
    assert lay.cell == 6 and tex.dtype == torch.uint8 and tuple(tex.shape) == (512, 512, 3)
    assert seen.dtype == torch.int32 and tuple(seen.shape) == (lay.n_texels,)
    _, _, face = atlas.texel_points(v, f, n, lay)
    live = face >= 0
    assert live.all() and (seen[live] > 0).all()
    truth, n0 = texel_truth(lay, f, colors, face)
    err = (texel_colours(tex, lay).double() - truth).abs().max(1).values
    print(f'sphere {kind}: texels with n0 >= 0 off by {int(err[n0 >= 0].max())}, gutter by {int(err[n0 < 0].max())}; seen min {int(seen.min())}')
    assert int(err[n0 >= 0].max()) <= 2


# ---- 5. held-out views --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size,bound', [(512, 2), (336, 3)])
@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
def test_held_out_views_show_the_true_colours(kind, size, bound):
    """Five cameras the bake has not seen, 128^2, ambient = 1: the textured render against the render in the true vertex colours, on
    mesh pixels.  Measured (orthographic / pinhole): largest difference 1 / 1 level at size 512 (mean 0.12 / 0.12), 2 / 2 at size 336
    (cell 4, side 1; mean 0.06 / 0.03); the bounds are one level above."""
    v, f, colors, _ = oriented('sphere')
    lay, tex, _ = baked('sphere', kind, size)
    cam = camera_kinds(4.2647)[kind][1]
    poses = fib_cameras(5, 1.0 if kind == 'ortho' else 2.7)
    got = atlas.render_textured(v, f, poses, cam, 128, tex, lay, ambient=1.0)
    want, fid, _ = mesh.render(v, f, poses, cam, 128, colors=colors, ambient=1.0, return_buffers=True)
    on = fid >= 0
    diff = (got.int() - want.int()).abs()
    print(f'held out {kind} size {size}: max {int(diff[on].max())}, mean {float(diff[on].float().mean()):.3f} on {int(on.sum())} pixels')
    assert int(on.sum()) > 20_000 and torch.equal(got[~on], want[~on])
    assert int(diff[on].max()) <= bound


# ---- 6. occlusion -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
def test_depth_test_keeps_the_two_spheres_apart_in_the_texture(kind):
    """Measured (orthographic / pinhole), size 256 (cell 5): 0.995 / 0.989 of the texels with n0 >= 0 seen, their largest error 3 levels;
    with the depth test disabled 0.37 / 0.42 of them are off by more than 8 levels."""
    v, f, colors, n = oriented('two')
    poses, cam, frames = scene_views('two', kind)
    lay, tex, seen = baked('two', kind, 256)
    _, _, face = atlas.texel_points(v, f, n, lay)
    truth, n0 = texel_truth(lay, f, colors, face)
    inner = (face >= 0) & (n0 >= 0)
    err = (texel_colours(tex, lay).double() - truth).abs().max(1).values
    hit = inner & (seen > 0)
    share = float(hit.sum()) / float(inner.sum())
    print(f'occlusion {kind}: seen share {share:.4f}, max error of seen {int(err[hit].max())}')
    assert share >= 0.98
    assert int(err[hit].max()) <= 8
    loose, _ = atlas.bake_texture(v, f, frames, poses, cam, lay, normals=n, tolerance=1e9)
    off = float(((texel_colours(loose, lay).double() - truth).abs().max(1).values[inner] > 8).float().mean())
    print(f'occlusion {kind}: without the depth test {off:.4f} of the texels are off by more than 8 levels')
    assert off > 0.25


# ---- 7. constant frames ---------------------------------------------------------------------------------------------------------------
def test_constant_frames_give_that_colour_on_every_seen_texel():
    v, f, _, n = oriented('two')
    poses, cam, frames = scene_views('two', 'pinhole')
    flat = torch.empty_like(frames)
    flat[:] = torch.tensor([37, 142, 251], dtype=torch.uint8)
    lay = atlas.layout(len(f), 256)
    tex, seen = atlas.bake_texture(v, f, flat, poses, cam, lay, normals=n, fallback=(1, 2, 3), background=(9, 9, 9))
    got = texel_colours(tex, lay)
    assert (seen > 0).sum() > 20_000 and (got[seen > 0] == torch.tensor([37, 142, 251], dtype=torch.uint8)).all()
    assert (seen == 0).any() and (got[seen == 0] == torch.tensor([1, 2, 3], dtype=torch.uint8)).all()
    used = lay.n_cells // lay.per_row * lay.cell                              # full rows of cells; below and right of them: background
    assert (tex[:, lay.per_row * lay.cell:] == 9).all() and (tex[used + lay.cell:] == 9).all() and not (tex[:used] == 9).all()


# ---- 8. grouping ----------------------------------------------------------------------------------------------------------------------
def test_one_view_per_group_gives_the_bytes_of_one_group():
    v, f, _, n = oriented('two')
    poses, cam, frames = scene_views('two', 'pinhole')
    lay, tex, seen = baked('two', 'pinhole', 256)
    for max_bytes in (1, 3 * 16 * lay.n_texels):
        t2, s2 = atlas.bake_texture(v, f, frames, poses, cam, 256, normals=n, max_bytes=max_bytes)
        assert torch.equal(t2, tex) and torch.equal(s2, seen)
    assert int(seen.max()) > 1


def test_render_textured_in_groups_of_views_gives_the_bytes_of_one_group():
    v, f, _, poses, cam = grouped_views()
    lay = atlas.layout(len(f), 256)
    tex = torch.randint(0, 256, [256, 256, 3], generator=torch.Generator().manual_seed(8), dtype=torch.uint8)

    def render(poses, camera, **kw):
        return atlas.render_textured(v, f, poses, camera, 96, tex, lay, **kw)
    check_view_groups(render, len(v), lambda k: render(poses[k:k + 1], mesh.Pinhole(cam.intrinsics[k])))


def test_render_textured_names_an_intrinsics_count_that_fits_no_frame_count():
    v, f, _, poses, cam = grouped_views()
    tex = torch.zeros([256, 256, 3], dtype=torch.uint8)
    with pytest.raises(ValueError, match='render_textured: 2 intrinsics for 3 frames'):
        atlas.render_textured(v, f, poses, mesh.Pinhole(cam.intrinsics[:2]), 96, tex, 256)


# ---- 9. the textured shade --------------------------------------------------------------------------------------------------------------
def loop_shade_textured(face_id, proj, vertices, faces, poses, tex, lay, ambient, background):
    """include/p3d_hip.h's textured shade, one pixel at a time in Python floats."""
    n, h, w = face_id.shape
    packed, fid, v, f, img = proj.packed.tolist(), face_id.tolist(), vertices.double().tolist(), faces.tolist(), tex.tolist()
    c2w = poses.double().reshape(-1, 4, 4).tolist()
    amb = float(torch.tensor(ambient, dtype=torch.float32))
    out = torch.empty([n, h, w, 3], dtype=torch.uint8)
    out[:] = torch.tensor(background, dtype=torch.uint8)
    cell, m, top = lay.cell, lay.cell - 3, lay.cell - 1
    swaps = 0
    for k in range(n):
        for r in range(h):
            for c in range(w):
                t = fid[k][r][c]
                if t < 0:
                    continue
                ids = list(f[t])
                rec = [packed[k][i] for i in ids]
                x, y = [p[0] for p in rec], [p[1] for p in rec]
                z = [float(np.array(p[2], dtype=np.int32).view(np.float32)) for p in rec]
                order = [0, 1, 2]
                if (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]) < 0:
                    order = [0, 2, 1]
                    swaps += 1
                x, y, z, ids = [x[o] for o in order], [y[o] for o in order], [z[o] for o in order], [ids[o] for o in order]
                px, py = (c << 8) + 128, (r << 8) + 128
                wts = [(x[2] - x[1]) * (py - y[1]) - (y[2] - y[1]) * (px - x[1]), (x[0] - x[2]) * (py - y[2]) - (y[0] - y[2]) * (px - x[2]),
                       (x[1] - x[0]) * (py - y[0]) - (y[1] - y[0]) * (px - x[0])]
                if proj.orthographic:
                    s = float(wts[0]) + float(wts[1]) + float(wts[2])
                    b = [float(a) / s for a in wts]
                else:
                    q = [float(a) / zz for a, zz in zip(wts, z)]
                    s = q[0] + q[1] + q[2]
                    b = [a / s for a in q]
                stored = [b[order.index(j)] for j in range(3)]                  # back into the face's own corner order
                e1 = [v[ids[1]][d] - v[ids[0]][d] for d in range(3)]
                e2 = [v[ids[2]][d] - v[ids[0]][d] for d in range(3)]
                nrm = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
                fwd = [c2w[k][0][2], c2w[k][1][2], c2w[k][2][2]]
                dot = nrm[0] * fwd[0] + nrm[1] * fwd[1] + nrm[2] * fwd[2]
                den = math.sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]) * math.sqrt(fwd[0] * fwd[0] + fwd[1] * fwd[1] + fwd[2] * fwd[2])
                shade = amb + (1.0 - amb) * (abs(dot) / den if den > 0 else 0.0)
                tx, ty = stored[1] * float(m), stored[2] * float(m)
                if t & 1:
                    tx, ty = float(top) - tx, float(top) - ty
                X, Y = min(max(round(tx * 256.0), 0), top * 256), min(max(round(ty * 256.0), 0), top * 256)      # round(): half to even
                c0, r0 = min(X >> 8, cell - 2), min(Y >> 8, cell - 2)
                fx, fy = X - (c0 << 8), Y - (r0 << 8)
                row, col = (t >> 1) // lay.per_row * cell + r0, (t >> 1) % lay.per_row * cell + c0
                for ch in range(3):
                    num = (256 - fy) * (256 - fx) * img[row][col][ch] + (256 - fy) * fx * img[row][col + 1][ch] + \
                        fy * (256 - fx) * img[row + 1][col][ch] + fy * fx * img[row + 1][col + 1][ch]
                    out[k, r, c, ch] = min(255, max(0, math.floor(num / 65536.0 * shade + 0.5)))
    return out, swaps


def shade_case(kind):
    """A 33 x 47 view of the two spheres with a random texture: both halves and swapped faces are on screen."""
    v, f, _, _ = oriented('two')
    f = f.clone()
    f[::3] = f[::3][:, [0, 2, 1]]                                             # every third face wound the other way: a closed mesh alone swaps all or none
    if kind == 'ortho':
        poses, cam = fib_cameras(14, 1.0)[3:5], mesh.Orthographic(0.4, 0.4)
    else:
        poses, cam = fib_cameras(14, 2.7)[3:5], mesh.Pinhole(torch.tensor([[3.2, 0, 0.5], [0, 3.2, 0.5], [0, 0, 1]]))
    lay = atlas.layout(len(f), 256)
    tex = torch.randint(0, 256, [256, 256, 3], generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    proj = mesh.project(v, poses, cam, (33, 47))
    fid, _ = mesh.rasterize(proj, f, (33, 47))
    return fid, proj, v, f, poses, tex, lay


@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
def test_textured_shade_equals_a_per_pixel_loop(kind):
    fid, proj, v, f, poses, tex, lay = shade_case(kind)
    on = fid[fid >= 0]
    assert len(on) > 300 and (on % 2 == 0).sum() > 50 and (on % 2 == 1).sum() > 50          # both halves
    for ambient in (1.0, 0.25):
        got = atlas.shade_textured(fid, proj, v, f, poses, tex, lay, background=(10, 255, 0), ambient=ambient)
        want, swaps = loop_shade_textured(fid, proj, v, f, poses, tex, lay, ambient, (10, 255, 0))
        assert swaps > 50 and swaps < len(on) - 50                              # faces the rasterizer swaps, and faces it does not
        assert got.dtype == torch.uint8 and torch.equal(got, want)
    assert (got[fid < 0] == torch.tensor([10, 255, 0], dtype=torch.uint8)).all()


# ---- 10. OBJ --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_normals', [True, False])
def test_write_obj_round_trips(tmp_path, with_normals):
    from PIL import Image
    v, f, _, n = oriented('two')
    f = f[:301]
    lay = atlas.layout(len(f), 100)
    tex = torch.randint(0, 256, [100, 100, 3], generator=torch.Generator().manual_seed(6), dtype=torch.uint8)
    path = tmp_path / 'two.obj'
    atlas.write_obj(path, v, f, lay, tex, normals=n if with_normals else None)
    rows = [line.split() for line in open(path).read().splitlines()]
    assert ['mtllib', 'two.mtl'] in rows and ['usemtl', 'atlas'] in rows
    assert rows.index(['usemtl', 'atlas']) < min(i for i, r in enumerate(rows) if r[0] == 'f')
    pv = torch.tensor([[float(x) for x in r[1:]] for r in rows if r[0] == 'v'], dtype=torch.float64).float()
    vt = torch.tensor([[float(x) for x in r[1:]] for r in rows if r[0] == 'vt'], dtype=torch.float64)
    vn = [r for r in rows if r[0] == 'vn']
    faces = [[[int(x) for x in c.split('/')] for c in r[1:]] for r in rows if r[0] == 'f']
    assert torch.equal(pv, v) and tuple(vt.shape) == (3 * len(f), 2) and len(faces) == len(f) and len(vn) == (len(v) if with_normals else 0)
    if with_normals:
        assert torch.equal(torch.tensor([[float(x) for x in r[1:]] for r in vn], dtype=torch.float64).float(), n)
    m, top = lay.side, lay.cell - 1
    for t, corners in enumerate(faces):
        assert all(len(c) == (3 if with_normals else 2) for c in corners)
        assert [c[0] - 1 for c in corners] == f[t].tolist() and all(1 <= c[0] <= len(v) for c in corners)       # 1-based and in range
        assert [c[1] for c in corners] == [3 * t + 1, 3 * t + 2, 3 * t + 3] and (not with_normals or all(c[2] == c[0] for c in corners))
        at = [(0, 0), (m, 0), (0, m)] if t % 2 == 0 else [(top, top), (top - m, top), (top, top - m)]
        for (i, j), c in zip(at, corners):
            u, w = vt[c[1] - 1].tolist()
            x, y = u * lay.size - 0.5, (1 - w) * lay.size - 0.5                 # the texel whose centre the corner sits on
            assert abs(x - ((t // 2) % lay.per_row * lay.cell + i)) < 1e-4 and abs(y - ((t // 2) // lay.per_row * lay.cell + j)) < 1e-4
    assert torch.equal(atlas.face_uv(lay).reshape(-1, 2).double(), vt.float().double())
    assert open(tmp_path / 'two.mtl').read().split() == ['newmtl', 'atlas', 'Kd', '1', '1', '1', 'map_Kd', 'two.png']
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'two.png').convert('RGB')), tex.numpy())
    with pytest.raises(ValueError, match='.obj'):
        atlas.write_obj(tmp_path / 'two.ply', v, f, lay, tex)
    with pytest.raises(ValueError, match='texture'):
        atlas.write_obj(path, v, f, lay, tex[:50])
    with pytest.raises(ValueError, match='layout'):
        atlas.write_obj(path, v, f[:100], lay, tex)


# ---- 11. argument checks and a CPU generator --------------------------------------------------------------------------------------------
def test_entry_points_reject_what_they_cannot_hold():
    """Argument checks of csrc/mesh_atlas.hip: error codes and messages, returned before any launch (no GPU needed)."""
    from pix2pix3d_amd import _lib
    h = _lib.lib()
    d = ctypes.c_void_p(16)
    big = 2 ** 31 - 1

    def texels(nv=8, nf=8, size=64, cell=32, faces=d):
        return h.p3d_mesh_atlas_texels(d, nv, faces, nf, d, size, cell, d, d, d, None)
    assert texels(nf=big) == -1 and b'INT32_MAX - 1 faces' in h.p3d_last_error()
    assert texels(nv=big) == -1 and b'INT32_MAX - 1 vertices' in h.p3d_last_error()
    assert texels(nf=-1) == -2 and texels(nv=-1) == -2
    assert texels(size=15) == -2 and texels(size=8193) == -2 and b'atlas size' in h.p3d_last_error()
    assert texels(cell=3) == -2 and texels(cell=65) == -2 and b'cell' in h.p3d_last_error()
    assert texels(nf=9) == -2 and b'need 5 cells' in h.p3d_last_error()
    assert texels(faces=None) == -2 and b'null pointer' in h.p3d_last_error()
    assert texels(nf=0) == 0                                                   # nothing to do: no launch

    def assemble(nf=8, size=64, cell=32, out=d):
        return h.p3d_mesh_atlas_assemble(d, d, nf, size, cell, 1, 2, 3, out, None)
    assert assemble(nf=big) == -1 and assemble(size=15) == -2 and assemble(cell=3) == -2 and assemble(nf=9) == -2
    assert assemble(out=None) == -2 and b'null pointer' in h.p3d_last_error()

    def shade(nv=8, nf=8, size=64, cell=32, n=2, w=64, hh=64, tex=d):
        return h.p3d_mesh_shade_textured(d, d, d, nv, d, nf, tex, size, cell, d, n, 0, w, hh, 0.3, 1, 2, 3, d, None)
    assert shade(nf=big) == -1 and shade(size=8193) == -2 and shade(cell=3) == -2 and shade(nf=9) == -2 and b'cells' in h.p3d_last_error()
    assert shade(nv=-1) == -2 and shade(n=65536) == -2 and b'65535' in h.p3d_last_error()
    assert shade(w=2049) == -2 and shade(hh=0) == -2 and b'image size' in h.p3d_last_error()
    assert shade(tex=None) == -2 and b'null pointer' in h.p3d_last_error()
    assert shade(n=0) == 0


def test_python_functions_check_their_arguments():
    v, f, _, n = oriented('two')
    poses, cam, frames = scene_views('two', 'ortho')
    lay = atlas.layout(len(f), 256)
    with pytest.raises(ValueError, match='13 cameras for 14 frames'):
        atlas.bake_texture(v, f, frames, poses[:13], cam, lay)
    with pytest.raises(ValueError, match='uint8'):
        atlas.bake_texture(v, f, frames.float(), poses, cam, lay)
    with pytest.raises(ValueError, match='smallest size'):
        atlas.bake_texture(v, f, frames, poses, cam, 128)
    with pytest.raises(ValueError, match='not the layout'):
        atlas.bake_texture(v, f, frames, poses, cam, atlas.layout(len(f) - 2, 256))
    with pytest.raises(ValueError, match='not the layout'):
        atlas.bake_texture(v, f, frames, poses, cam, lay._replace(cell=4, per_row=64))
    for bad in (dict(power=0), dict(power=1.5), dict(tolerance=-1.0), dict(min_cos=math.inf)):
        with pytest.raises(ValueError, match='bake'):
            atlas.bake_texture(v, f, frames, poses, cam, lay, **bad)
    with pytest.raises(ValueError, match='fallback'):
        atlas.bake_texture(v, f, frames, poses, cam, lay, fallback=torch.zeros([len(v), 3], dtype=torch.uint8))
    with pytest.raises(ValueError, match='background'):
        atlas.bake_texture(v, f, frames, poses, cam, lay, background=(0, 0, 256))
    with pytest.raises(ValueError, match='normals'):
        atlas.bake_texture(v, f, frames, poses, cam, lay, normals=n[:-1])
    with pytest.raises(ValueError, match='face index'):
        atlas.bake_texture(v, f + 1, frames, poses, cam, lay)
    with pytest.raises(ValueError, match='normals'):
        atlas.texel_points(v, f, n[:-1], lay)
    proj = mesh.project(v, poses[:2], cam, 32)
    fid, _ = mesh.rasterize(proj, f, 32)
    tex = torch.zeros([256, 256, 3], dtype=torch.uint8)
    with pytest.raises(ValueError, match='texture'):
        atlas.shade_textured(fid, proj, v, f, poses[:2], tex[:128], lay)
    with pytest.raises(ValueError, match='texture'):
        atlas.shade_textured(fid, proj, v, f, poses[:2], tex.float(), lay)
    with pytest.raises(ValueError, match='3 cameras for 2 frames'):
        atlas.shade_textured(fid, proj, v, f, poses[:3], tex, lay)
    with pytest.raises(ValueError, match='not the layout'):
        atlas.shade_textured(fid, proj, v, f[:-1], poses[:2], tex, lay)
    with pytest.raises(ValueError, match='assemble'):
        atlas.assemble(torch.zeros([5, 3], dtype=torch.uint8), torch.zeros([5], dtype=torch.int32), lay)


@pytest.mark.parametrize('with_path', [True, False])
def test_atlas_mesh_on_a_cpu_generator(tmp_path, with_path):
    G, ws, thr = small_generator('seg2cat')
    path = tmp_path / 'cat.obj'
    torch.manual_seed(11)
    v, f, lay, tex, seen, frames = atlas.atlas_mesh(G, ws, 'seg2cat', size=256, resolution=32, threshold=thr, n_frames=2, image_size=64,
                                                    cell=0.08, n_views=1, path=str(path) if with_path else None,
                                                    render_kwargs=dict(neural_rendering_resolution=16))
    assert len(f) > 1000 and lay == atlas.layout(len(f), 256) and lay.cell >= 5 and torch.equal(atlas.orient_faces(v, f), f)
    assert tex.dtype == torch.uint8 and tuple(tex.shape) == (256, 256, 3) and seen.dtype == torch.int32 and tuple(seen.shape) == (lay.n_texels,)
    assert tuple(frames.shape) == (2, 64, 64, 3) and frames.dtype == torch.uint8
    assert (seen > 0).any() and (seen == 0).any() and int(seen.max()) == 1        # one view: the generator's frames are what costs time here
    pts, _, face = atlas.texel_points(v, f, texture.vertex_normals(v, f), lay)
    unseen = (seen == 0) & (face >= 0)
    assert torch.equal(texel_colours(tex, lay)[unseen], texture.vertex_rgb(G, ws, pts)[unseen])      # the decoder's own colour
    poses, camera = mesh.script_turntable(G, 2)
    assert torch.equal(frames, atlas.render_textured(v, f, poses, camera, 64, tex, lay))
    assert not torch.equal(frames, mesh.render(v, f, poses, camera, 64))
    assert sorted(p.name for p in tmp_path.iterdir()) == (['cat.mtl', 'cat.obj', 'cat.png'] if with_path else [])
    if not with_path:
        with pytest.raises(ValueError, match='smallest size'):               # too many faces for the image: said before any view is rendered
            atlas.atlas_mesh(G, ws, 'seg2cat', size=256, resolution=32, threshold=thr, n_frames=2, image_size=64, n_views=3)
