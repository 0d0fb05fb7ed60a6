"""Vertex normals and colour baking (pix2pix3d_amd/texture.py), CPU formulation: against per-vertex Python loops, round trips of known
colours through rendered frames, the occlusion test, view groups, the PLY with normals, argument checks, a CPU generator."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

from pix2pix3d_amd import configs, mesh, shape, texture
from test_mesh_host import grid_mesh, random_soup
from test_shape_host import sphere


def _f32(bits):
    return struct.unpack('<f', struct.pack('<i', int(bits)))[0]


# ---- scenes shared with test_texture_gpu.py ------------------------------------------------------------------------------------
def fib_cameras(n, radius):
    """float32 [n, 4, 4]: n cameras on a Fibonacci sphere of ``radius`` looking at the origin."""
    out = []
    for k in range(n):
        y = 1 - 2 * (k + 0.5) / n
        phi = k * math.pi * (3 - math.sqrt(5))
        r = math.sqrt(1 - y * y)
        out.append(configs.look_at(radius * np.array([math.cos(phi) * r, y, math.sin(phi) * r]), np.zeros(3)))
    return torch.from_numpy(np.stack(out)).to(torch.float32)


def camera_kinds(focal, n=14):
    k = torch.tensor([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]], dtype=torch.float32)
    return {'ortho': (fib_cameras(n, 1.0), mesh.Orthographic(0.55, 0.55)), 'pinhole': (fib_cameras(n, 2.7), mesh.Pinhole(k))}


def true_colors(p):
    s = torch.sin(p.double() * torch.tensor([9.0, 7.0, 11.0], dtype=torch.float64) + torch.tensor([0.3, 1.1, 2.0], dtype=torch.float64))
    return torch.round(127.5 + 100 * s).to(torch.uint8)


_scenes = {}


def sphere_scene():
    """The 48^3 sphere of radius 19.2 in the unit box with smooth true colours."""
    if 'sphere' not in _scenes:
        v, f = shape.marching_cubes(sphere(48, 19.2), 0.0)
        v = v / 47 - 0.5
        _scenes['sphere'] = (v, f, true_colors(v))
    return _scenes['sphere']


def two_sphere_scene():
    """Two spheres of radius 7 on a 40^3 lattice, one red, one blue (by nearer centre)."""
    if 'two' not in _scenes:
        ca, cb = [12.2, 19.4, 19.7], [27.3, 19.6, 19.2]
        v, f = shape.marching_cubes(torch.maximum(sphere(40, 7.0, ca), sphere(40, 7.0, cb)), 0.0)
        first = (v - torch.tensor(ca)).norm(dim=1) < (v - torch.tensor(cb)).norm(dim=1)
        colors = torch.where(first[:, None], torch.tensor([220, 40, 30]), torch.tensor([30, 60, 230])).to(torch.uint8)
        _scenes['two'] = (v / 39 - 0.5, f, colors)
    return _scenes['two']


def flat_frames(v, f, colors, poses, camera, size):
    """Frames of the mesh in its true colours: ambient = 1 makes the shading factor exactly 1."""
    return mesh.render(v, f, poses, camera, size, colors=colors, ambient=1.0)


def soup_inputs(seed, h, w, n_frames=3, ortho=False):
    """random_soup-like inputs of a bake that need not be a consistent scene: per frame the projected records of a soup (dropped
    vertices, vertices off the frame) with its own raster buffers, random frames, positions, normals and poses; the last vertex is
    used by no face and vertex 0 has a zero normal."""
    g = torch.Generator().manual_seed(seed)
    packed, fid, dep = [], [], []
    for k in range(n_frames):
        p, faces = random_soup(seed * 10 + k, h, w)
        p = torch.cat([p, torch.tensor([[w * 128, h * 128, p[0, 2], 0]], dtype=torch.int32)])          # the unused vertex, mid-frame
        proj = mesh.Projection(p[None], ortho)
        a, b = mesh.rasterize(proj, faces, (h, w))
        packed.append(p); fid.append(a[0]); dep.append(b[0])
    nv = packed[0].shape[0]
    vertices = torch.rand([nv, 3], generator=g) - 0.5
    normals = torch.nn.functional.normalize(torch.randn([nv, 3], generator=g), dim=1)
    normals[0] = 0
    poses = fib_cameras(n_frames, 2.0)
    images = torch.randint(0, 256, [n_frames, h, w, 3], generator=g, dtype=torch.uint8)
    return mesh.Projection(torch.stack(packed), ortho), torch.stack(fid), torch.stack(dep), images, vertices, normals, poses


# ---- 1. independent loops ---------------------------------------------------------------------------------------------------------
def loop_normals(vertices, faces):
    v = [[float(x) for x in row] for row in vertices.tolist()]
    acc = [[0.0, 0.0, 0.0] for _ in v]
    for a, b, c in faces.tolist():                                          # ascending face id, and a face's corners in order
        e1 = [v[b][k] - v[a][k] for k in range(3)]
        e2 = [v[c][k] - v[a][k] for k in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        for corner in (a, b, c):
            for k in range(3):
                acc[corner][k] = acc[corner][k] + n[k]
    out = torch.zeros([len(v), 3], dtype=torch.float32)
    for i, (x, y, z) in enumerate(acc):
        length = math.sqrt(x * x + y * y + z * z)
        if length > 0 and math.isfinite(length):
            out[i] = torch.tensor([x / length, y / length, z / length], dtype=torch.float64).float()
    return out


def loop_bake(proj, face_id, depth, images, vertices, normals, poses, tolerance, power, min_cos, fallback):
    """include/p3d_hip.h's baking rules, one vertex and one view at a time in Python floats (IEEE doubles, one rounding per operation)."""
    packed = proj.packed.tolist()
    n_frames, nv = proj.packed.shape[:2]
    h, w = face_id.shape[1:]
    fid, dep, img = face_id.tolist(), depth.double().tolist(), images.tolist()
    c2w = poses.double().reshape(-1, 4, 4).tolist()
    colors, seen = torch.zeros([nv, 3], dtype=torch.uint8), torch.zeros([nv], dtype=torch.int32)
    for v in range(nv):
        p = [float(x) for x in vertices[v].tolist()]
        n = [float(x) for x in normals[v].tolist()]
        acc, count = [0.0, 0.0, 0.0, 0.0], 0
        for f in range(n_frames):
            sx, sy, zbits, dropped = packed[f][v]
            tx, ty = sx - 128, sy - 128
            c0, r0, fx, fy = tx >> 8, ty >> 8, tx & 255, ty & 255
            if dropped or c0 < 0 or r0 < 0 or c0 + 1 > w - 1 or r0 + 1 > h - 1:
                continue
            taps = [(r0, c0), (r0, c0 + 1), (r0 + 1, c0), (r0 + 1, c0 + 1)]
            if any(fid[f][r][c] < 0 for r, c in taps):
                continue
            if not _f32(zbits) <= min(dep[f][r][c] for r, c in taps) + tolerance:
                continue
            m = c2w[f]
            d = [-m[0][2], -m[1][2], -m[2][2]] if proj.orthographic else [m[0][3] - p[0], m[1][3] - p[1], m[2][3] - p[2]]
            dot = n[0] * d[0] + n[1] * d[1] + n[2] * d[2]
            den = math.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) * math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            cos = abs(dot) / den if den > 0 else 0.0
            if not cos >= min_cos:
                continue
            wgt = cos
            for _ in range(power - 1):
                wgt = wgt * cos
            wts = [(256 - fy) * (256 - fx), (256 - fy) * fx, fy * (256 - fx), fy * fx]
            for ch in range(3):
                num = sum(wt * img[f][r][c][ch] for wt, (r, c) in zip(wts, taps))
                acc[ch] = acc[ch] + wgt * (num / 65536.0)
            acc[3] = acc[3] + wgt
            count += 1
        seen[v] = count
        if acc[3] > 0:
            colors[v] = torch.tensor([min(255, math.floor(acc[ch] / acc[3] + 0.5)) for ch in range(3)], dtype=torch.uint8)
        else:
            colors[v] = torch.as_tensor(fallback[v] if torch.is_tensor(fallback) and fallback.ndim == 2 else fallback, dtype=torch.uint8)
    return colors, seen


def run_bake(device, proj, face_id, depth, images, vertices, normals, poses, tolerance, power, min_cos, fallback, groups=None):
    """bake_accumulate over the given groups of views (default: one group of all), then bake_finish, on ``device``."""
    acc, seen = texture.bake_buffers(vertices.shape[0], device)
    n = images.shape[0]
    for s, e in groups or [(0, n)]:
        part = mesh.Projection(proj.packed[s:e], proj.orthographic)
        texture.bake_accumulate(acc, seen, part, face_id[s:e], depth[s:e], images[s:e], vertices, normals, poses[s:e], tolerance, power, min_cos)
    return texture.bake_finish(acc, fallback), seen, acc


def test_vertex_normals_equal_a_per_vertex_loop():
    packed, faces = grid_mesh(1, 40, 52)
    g = torch.Generator().manual_seed(0)
    v = torch.cat([packed[:, :2].float() / 256, torch.rand([len(packed), 1], generator=g) * 9], dim=1)
    v = torch.cat([v, torch.tensor([[1.0, 2.0, 3.0]])])                    # a vertex no face uses
    faces = torch.cat([faces, torch.tensor([[3, 3, 7], [5, 9, 5]])])       # degenerate faces: a corner listed twice, a zero cross product
    got = texture.vertex_normals(v, faces)
    assert got.dtype == torch.float32 and torch.equal(got, loop_normals(v, faces))
    assert torch.equal(got[-1], torch.zeros(3)) and (got[:-1].norm(dim=1) - 1).abs().max() < 1e-6
    v, f = shape.marching_cubes(sphere(12, 4.3), 0.0)
    got = texture.vertex_normals(v, f)
    assert torch.equal(got, loop_normals(v, f))
    centre = torch.tensor([5.67, 5.27, 5.55])
    outward = torch.nn.functional.normalize(v - centre, dim=1)
    assert ((got * outward).sum(1).abs() > 0.9).all()                       # they are the sphere's normals


@pytest.mark.parametrize('ortho,power,min_cos,tolerance', [(False, 2, 0.1, 0.4), (True, 1, 0.0, 0.05), (False, 3, 0.5, 1e9)])
def test_bake_equals_a_per_vertex_per_view_loop(ortho, power, min_cos, tolerance):
    h, w = 33, 47
    proj, fid, dep, images, v, n, poses = soup_inputs(3, h, w, ortho=ortho)
    assert proj.dropped.any() and (proj.packed[..., 0] < 0).any() and (proj.packed[..., 1] > h * 256).any()
    fallback = torch.randint(0, 256, [len(v), 3], generator=torch.Generator().manual_seed(1), dtype=torch.uint8) if ortho else (1, 2, 3)
    colors, seen, _ = run_bake('cpu', proj, fid, dep, images, v, n, poses, tolerance, power, min_cos, fallback)
    want, want_seen = loop_bake(proj, fid, dep, images, v, n, poses, tolerance, power, min_cos, fallback)
    assert torch.equal(seen, want_seen) and torch.equal(colors, want)
    assert (seen > 0).sum() > 20 and (seen == 0).sum() > 20 and seen.max() >= 2


def test_bake_colors_equals_the_loop_on_small_meshes_and_no_frames():
    # V = 1, F = 1: a single vertex has no faces, so nothing covers it and it takes the fallback; with a triangle around it, it is seen
    one = torch.tensor([[0.1, -0.05, 0.0]])
    img = torch.randint(0, 256, [1, 33, 47, 3], generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    pose, cam = fib_cameras(1, 1.0), mesh.Orthographic(0.55, 0.55)
    colors, seen = texture.bake_colors(one, torch.zeros([0, 3], dtype=torch.int64), img, pose, cam, normals=torch.tensor([[0.0, 1.0, 0.0]]),
                                       fallback=(9, 8, 7), return_seen=True)
    assert colors.tolist() == [[9, 8, 7]] and seen.tolist() == [0]
    tri = torch.cat([one, one + torch.tensor([[0.0, 0.3, 0.1], [0.0, -0.1, -0.4], [0.0, -0.3, 0.2]])])
    faces = torch.tensor([[1, 2, 3], [0, 1, 2]])
    colors, seen = texture.bake_colors(tri, faces, img, pose, cam, tolerance=0.5, min_cos=0.0, return_seen=True)
    proj = mesh.project(tri, pose, cam, (33, 47))
    fid, dep = mesh.rasterize(proj, faces, (33, 47))
    want, want_seen = loop_bake(proj, fid, dep, img, tri, texture.vertex_normals(tri, faces), pose, 0.5, 2, 0.0, (200, 200, 200))
    assert torch.equal(colors, want) and torch.equal(seen, want_seen) and seen[0] == 1
    # F = 0: every vertex gets the fallback
    v, f, _ = two_sphere_scene()
    fb = torch.randint(0, 256, [len(v), 3], generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    colors, seen = texture.bake_colors(v, f, torch.zeros([0, 16, 16, 3], dtype=torch.uint8), torch.zeros([0, 4, 4]), cam, fallback=fb,
                                       return_seen=True)
    assert torch.equal(colors, fb) and int(seen.sum()) == 0
    assert torch.equal(texture.bake_colors(v, f, torch.zeros([0, 16, 16, 3], dtype=torch.uint8), torch.zeros([0, 4, 4]), cam),
                       torch.full([len(v), 3], 200, dtype=torch.uint8))


# ---- 2. round trip ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
def test_round_trip_of_known_colours_through_frames(kind):
    """Measured with this formulation: every vertex seen; largest error 1 level in both camera kinds; mean error 0.040 (orthographic),
    0.006 (pinhole).  The bound of 2 levels is the prototype's measured 1 plus one level for rounding details."""
    v, f, colors = sphere_scene()
    poses, cam = camera_kinds(4.2647)[kind]
    frames = flat_frames(v, f, colors, poses, cam, 128)
    baked, seen = texture.bake_colors(v, f, frames, poses, cam, return_seen=True)
    err = (baked.int() - colors.int()).abs()
    print(f'round trip {kind}: seen min {int(seen.min())}, max error {int(err.max())}, mean error {float(err.float().mean()):.4f}')
    assert (seen > 0).all()
    assert int(err.max()) <= 2


# ---- 3. occlusion ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
def test_depth_test_keeps_two_spheres_apart(kind):
    """Measured with this formulation (orthographic / pinhole): seen share 0.997 / 0.990 and largest error 2 levels at the default
    tolerance; with the depth test disabled 37 % / 42 % of the vertices are off by more than 8 levels."""
    v, f, colors = two_sphere_scene()
    poses, cam = camera_kinds(2.2)[kind]
    frames = flat_frames(v, f, colors, poses, cam, 96)
    baked, seen = texture.bake_colors(v, f, frames, poses, cam, return_seen=True)
    err = (baked.int() - colors.int()).abs().max(dim=1).values
    hit = seen > 0
    print(f'occlusion {kind}: seen share {float(hit.float().mean()):.4f}, max error of seen {int(err[hit].max())}')
    assert float(hit.float().mean()) >= 0.98
    assert int(err[hit].max()) <= 8
    loose = texture.bake_colors(v, f, frames, poses, cam, tolerance=1e9)
    off = ((loose.int() - colors.int()).abs().max(dim=1).values > 8).float().mean()
    print(f'occlusion {kind}: without the depth test {float(off):.4f} of the vertices are off by more than 8 levels')
    assert float(off) > 0.25


# ---- 4. view groups -------------------------------------------------------------------------------------------------------------
def test_one_view_per_group_gives_the_bytes_of_one_group():
    v, f, colors = two_sphere_scene()
    poses, cam = camera_kinds(2.2)['pinhole']
    frames = flat_frames(v, f, colors, poses, cam, 64)
    a, sa = texture.bake_colors(v, f, frames, poses, cam, return_seen=True)
    b, sb = texture.bake_colors(v, f, frames, poses, cam, return_seen=True, max_bytes=1)
    assert torch.equal(a, b) and torch.equal(sa, sb) and int(sa.max()) > 1
    proj = mesh.project(v, poses, cam, 64)
    fid, dep = mesh.rasterize(proj, f, 64)
    n = texture.vertex_normals(v, f)
    whole = run_bake('cpu', proj, fid, dep, frames, v, n, poses, 0.01, 2, 0.1, (200, 200, 200))
    parts = run_bake('cpu', proj, fid, dep, frames, v, n, poses, 0.01, 2, 0.1, (200, 200, 200), groups=[(0, 1), (1, 6), (6, 14)])
    assert torch.equal(whole[2], parts[2]) and torch.equal(whole[1], parts[1]) and torch.equal(whole[0], a)


# ---- 5. PLY ---------------------------------------------------------------------------------------------------------------------
def _parent_ply_bytes(v, f, colors):
    """The bytes write_ply wrote before it took normals: header and records built again here."""
    props = 'property float x\nproperty float y\nproperty float z\n'
    if colors is not None:
        props += 'property uchar red\nproperty uchar green\nproperty uchar blue\n'
    out = (f'ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\n{props}element face {len(f)}\n'
           'property list uchar int vertex_indices\nend_header\n').encode('ascii')
    for i, p in enumerate(v.tolist()):
        out += struct.pack('<3f', *p) + (bytes(colors[i].tolist()) if colors is not None else b'')
    for t in f.tolist():
        out += struct.pack('<B3i', 3, *t)
    return out


def test_write_ply_with_normals_round_trips_and_without_is_unchanged(tmp_path):
    v, f = shape.marching_cubes(sphere(12, 4.3), 0.0)
    colors = torch.randint(0, 256, [len(v), 3], generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    normals = texture.vertex_normals(v, f)
    for c in (colors, None):
        path = tmp_path / 'plain.ply'
        mesh.write_ply(path, v, f, c)
        assert open(path, 'rb').read() == _parent_ply_bytes(v, f, c)
        path = tmp_path / 'normals.ply'
        mesh.write_ply(path, v, f, c, normals=normals)
        data = open(path, 'rb').read()
        end = data.index(b'end_header\n') + len(b'end_header\n')
        header = data[:end].decode('ascii').split('\n')
        names = [line.split()[-1] for line in header if line.startswith('property') and 'list' not in line]
        assert names == ['x', 'y', 'z', 'nx', 'ny', 'nz'] + (['red', 'green', 'blue'] if c is not None else [])
        vdt = [('p', '<f4', (3,)), ('n', '<f4', (3,))] + ([('c', 'u1', (3,))] if c is not None else [])
        vrec = np.frombuffer(data, dtype=vdt, count=len(v), offset=end)
        frec = np.frombuffer(data, dtype=[('k', 'u1'), ('i', '<i4', (3,))], count=len(f), offset=end + vrec.nbytes)
        assert end + vrec.nbytes + frec.nbytes == len(data)
        assert np.array_equal(vrec['p'], v.numpy()) and np.array_equal(vrec['n'], normals.numpy()) and np.array_equal(frec['i'], f.numpy())
        assert c is None or np.array_equal(vrec['c'], c.numpy())
    with pytest.raises(ValueError, match='normals'):
        mesh.write_ply(tmp_path / 'bad.ply', v, f, normals=normals[:-1])


# ---- 6. argument checks ---------------------------------------------------------------------------------------------------------
def test_entry_points_reject_what_they_cannot_hold():
    """Argument checks of csrc/mesh_bake.hip: error codes and messages, returned before any launch (no GPU needed)."""
    from pix2pix3d_amd import _lib
    h = _lib.lib()
    d = ctypes.c_void_p(16)
    big = 2 ** 31 - 1
    assert h.p3d_mesh_vertex_normals(d, big, d, 4, d, d, d, None) == -1 and b'INT32_MAX - 1 vertices' in h.p3d_last_error()
    assert h.p3d_mesh_vertex_normals(d, 4, d, big, d, d, d, None) == -1 and b'INT32_MAX - 1 faces' in h.p3d_last_error()
    assert h.p3d_mesh_vertex_normals(d, -1, d, 4, d, d, d, None) == -2
    assert h.p3d_mesh_vertex_normals(d, 4, d, 4, None, d, d, None) == -2 and b'null pointer' in h.p3d_last_error()

    def accumulate(nv=8, n=2, w=64, hh=64, tol=0.01, min_cos=0.1, power=2, acc=d):
        return h.p3d_mesh_bake_accumulate(d, d, d, d, d, d, d, nv, n, 0, w, hh, tol, min_cos, power, acc, d, None)
    assert accumulate(nv=big) == -1 and b'INT32_MAX - 1 vertices' in h.p3d_last_error()
    assert accumulate(n=65536) == -2 and b'65535' in h.p3d_last_error()
    assert accumulate(w=2049) == -2 and accumulate(hh=2049) == -2 and accumulate(w=0) == -2 and b'image size' in h.p3d_last_error()
    assert accumulate(power=0) == -2 and accumulate(power=9) == -2 and b'power' in h.p3d_last_error()
    assert accumulate(tol=-1.0) == -2 and accumulate(tol=math.inf) == -2 and accumulate(tol=math.nan) == -2 and b'tolerance' in h.p3d_last_error()
    assert accumulate(min_cos=-0.5) == -2 and accumulate(min_cos=math.nan) == -2 and b'min_cos' in h.p3d_last_error()
    assert accumulate(acc=None) == -2 and b'null pointer' in h.p3d_last_error()
    assert accumulate(n=0) == 0 and accumulate(nv=0) == 0 and accumulate(w=1) == 0        # nothing to do: no launch
    assert h.p3d_mesh_bake_finish(d, big, None, 1, 2, 3, d, None) == -1 and b'INT32_MAX - 1 vertices' in h.p3d_last_error()
    assert h.p3d_mesh_bake_finish(None, 4, None, 1, 2, 3, d, None) == -2 and b'null pointer' in h.p3d_last_error()
    assert h.p3d_mesh_bake_finish(d, 0, None, 1, 2, 3, d, None) == 0


def test_bake_colors_checks_its_arguments():
    v, f, colors = two_sphere_scene()
    poses, cam = camera_kinds(2.2)['ortho']
    frames = torch.zeros([14, 16, 16, 3], dtype=torch.uint8)
    with pytest.raises(ValueError, match='13 cameras for 14 frames'):
        texture.bake_colors(v, f, frames, poses[:13], cam)
    with pytest.raises(ValueError, match='uint8'):
        texture.bake_colors(v, f, frames.float(), poses, cam)
    with pytest.raises(ValueError, match='uint8'):
        texture.bake_colors(v, f, frames[..., :2], poses, cam)
    for bad in (dict(power=0), dict(power=9), dict(power=1.5), dict(tolerance=-1.0), dict(tolerance=math.nan), dict(min_cos=math.inf)):
        with pytest.raises(ValueError, match='bake'):
            texture.bake_colors(v, f, frames, poses, cam, **bad)
    with pytest.raises(ValueError, match='fallback'):
        texture.bake_colors(v, f, frames, poses, cam, fallback=colors[:-1])
    with pytest.raises(ValueError, match='normals'):
        texture.bake_colors(v, f, frames, poses, cam, normals=torch.zeros([3, 3]))


# ---- 7. a CPU generator ---------------------------------------------------------------------------------------------------------
def small_generator(name, device='cpu'):
    from model_cases import build_generator
    G = build_generator(name, device, cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0)
    ws = torch.randn([1, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(0)).to(device)
    thr = float(shape.sigma_grid(G, ws, 32)[0].median())
    return G, ws, thr


def test_vertex_rgb_and_bake_views_on_a_cpu_generator():
    G, ws, thr = small_generator('seg2cat')
    v, f = shape.extract_geometry(G, ws, 32, thr)
    assert len(f) > 100
    rgb = texture.vertex_rgb(G, ws, v)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (len(v), 3)
    with torch.no_grad():
        x = G.sample_mixed(v[None], None, ws, truncation_psi=1, noise_mode='const')['rgb'][0, :, :3] * 2 - 1
    assert torch.equal(rgb, ((x + 1) * 127.5).clamp(0, 255).to(torch.uint8))
    assert torch.equal(rgb, texture.vertex_rgb(G, ws, v, max_batch=1000))
    assert tuple(texture.bake_cameras(G, 'seg2cat', 3).shape) == (3, 25)
    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        runs.append(texture.bake_views(G, ws, v, f, 'seg2cat', n_views=3, render_kwargs=dict(neural_rendering_resolution=16)))
    colors, seen = runs[0]
    assert colors.dtype == torch.uint8 and tuple(colors.shape) == (len(v), 3) and seen.dtype == torch.int32 and tuple(seen.shape) == (len(v),)
    assert torch.equal(colors, runs[1][0]) and torch.equal(seen, runs[1][1])           # frozen jitter repeats
    assert 0 <= int(seen.min()) and int(seen.max()) <= 3 and (seen == 0).any() and (seen > 0).any()
    assert torch.equal(colors[seen == 0], rgb[seen == 0])
