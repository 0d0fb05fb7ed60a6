"""pix2pix3d_amd.mesh on the CPU: the vectorised rasterizer against a per-pixel loop, the fill rule, the camera models, the shading,
the turntable, the files, and a closed mesh rendered without holes."""
import math
import struct

import numpy as np
import pytest
import torch

from pix2pix3d_amd import mesh, shape
from test_shape_host import sphere


def _f32(bits):
    return struct.unpack('<f', struct.pack('<i', bits))[0]


def _bits(x):
    return struct.unpack('<I', struct.pack('<f', x))[0]


def brute_raster(packed, faces, h, w, ortho):
    """One frame, pixel by pixel and triangle by triangle in plain Python ints and floats: (face id [H][W], depth [H][W], coverage
    count [H][W]).  The conventions of include/p3d_hip.h, written out again."""
    P, F = packed.tolist(), faces.tolist()
    key = [[None] * w for _ in range(h)]
    count = [[0] * w for _ in range(h)]
    for t, tri in enumerate(F):
        if any(not 0 <= i < len(P) for i in tri) or any(P[i][3] for i in tri):
            continue
        x, y, z = [P[i][0] for i in tri], [P[i][1] for i in tri], [_f32(P[i][2]) for i in tri]
        area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
        if area == 0:
            continue
        if area < 0:
            x[1], x[2], y[1], y[2], z[1], z[2] = x[2], x[1], y[2], y[1], z[2], z[1]
        for r in range(h):
            for c in range(w):
                px, py = c * 256 + 128, r * 256 + 128
                ws, ok = [], True
                for a, b in ((1, 2), (2, 0), (0, 1)):
                    dx, dy = x[b] - x[a], y[b] - y[a]
                    e = dx * (py - y[a]) - dy * (px - x[a])
                    ok &= e > 0 or (e == 0 and (dy < 0 or (dy == 0 and dx > 0)))
                    ws.append(float(e))
                if not ok:
                    continue
                count[r][c] += 1
                s = ws[0] + ws[1] + ws[2]
                if ortho:
                    d = (ws[0] * z[0] + ws[1] * z[1]) + ws[2] * z[2]
                    d = d / s
                else:
                    q = (ws[0] / z[0] + ws[1] / z[1]) + ws[2] / z[2]
                    d = s / q
                k = (_bits(d) << 32) | t
                if key[r][c] is None or k < key[r][c]:
                    key[r][c] = k
    fid = torch.tensor([[-1 if k is None else k & 0xffffffff for k in row] for row in key], dtype=torch.int32)
    dep = torch.tensor([[math.inf if k is None else _f32(k >> 32 if (k >> 32) < 2 ** 31 else (k >> 32) - 2 ** 32) for k in row] for row in key])
    return fid, dep, torch.tensor(count)


def random_soup(seed, h, w, n=60):
    """Projected vertices (packed, as p3d_mesh_project writes them) of a soup with both windings, zero-area triangles, vertices on
    pixel centres and edges through them, triangles partly off screen and dropped vertices (a triangle crossing znear)."""
    g = torch.Generator().manual_seed(seed)
    nv = 3 * n
    x = torch.randint(-8 * 256, (w + 8) * 256, [nv], generator=g)
    y = torch.randint(-8 * 256, (h + 8) * 256, [nv], generator=g)
    snap = torch.rand([nv], generator=g) < 0.4                               # onto pixel centres
    x = torch.where(snap, (x >> 8 << 8) + 128, x)
    y = torch.where(snap, (y >> 8 << 8) + 128, y)
    small = torch.arange(nv) % 3 != 0                                        # many small triangles near their first vertex
    small &= torch.rand([nv], generator=g) < 0.5
    base = torch.arange(nv) // 3 * 3
    x = torch.where(small, x[base] + torch.randint(-700, 700, [nv], generator=g), x)
    y = torch.where(small, y[base] + torch.randint(-700, 700, [nv], generator=g), y)
    for t in range(0, n, 10):                                                # zero area: collinear on a pixel-centre row
        x[3 * t + 2], y[3 * t + 2] = (x[3 * t] + x[3 * t + 1]) // 2, y[3 * t]
        y[3 * t + 1] = y[3 * t]
    for t in range(5, n, 10):                                                # axis-aligned edges through pixel centres
        x[3 * t + 1], y[3 * t + 1] = x[3 * t], y[3 * t] + 256 * 5
        y[3 * t + 2] = y[3 * t]
        x[3 * t:3 * t + 3] = (x[3 * t:3 * t + 3] >> 8 << 8) + 128
        y[3 * t:3 * t + 3] = (y[3 * t:3 * t + 3] >> 8 << 8) + 128
    z = torch.rand([nv], generator=g) * 2 + 0.5
    z[7 * 3] = 0.75                                                          # exact depth ties between triangles
    z[7 * 3 + 1] = 0.75
    z[7 * 3 + 2] = 0.75
    z[8 * 3:8 * 3 + 3] = 0.75
    dropped = (torch.rand([nv], generator=g) < 0.04).to(torch.int32)
    x, y = torch.where(dropped.bool(), 0, x), torch.where(dropped.bool(), 0, y)
    packed = torch.stack([x.to(torch.int32), y.to(torch.int32), z.view(torch.int32), dropped], -1)
    faces = torch.arange(nv).reshape(n, 3)
    flip = torch.rand([n], generator=g) < 0.5                                # both windings
    faces[flip] = faces[flip][:, [0, 2, 1]]
    faces[3, 1] = nv + 5                                                     # an index out of range: not drawn
    return packed, faces


@pytest.mark.parametrize('seed,h,w', [(0, 32, 32), (1, 48, 40), (2, 40, 48), (3, 48, 48)])
@pytest.mark.parametrize('ortho', [True, False])
def test_raster_equals_per_pixel_loop(seed, h, w, ortho):
    packed, faces = random_soup(seed, h, w)
    proj = mesh.Projection(packed[None], ortho)
    fid, dep = mesh.rasterize(proj, faces, (h, w))
    bfid, bdep, _ = brute_raster(packed, faces, h, w, ortho)
    assert (bfid >= 0).sum() > h * w // 4
    assert torch.equal(fid[0], bfid)
    assert torch.equal(dep[0], bdep.to(torch.float32))


def test_projected_soup_crossing_znear_equals_per_pixel_loop():
    """A pinhole soup in front of and behind znear, through project: triangles with a vertex nearer than znear disappear whole."""
    g = torch.Generator().manual_seed(5)
    v = torch.rand([180, 3], generator=g) * torch.tensor([2.0, 2.0, 1.2]) - torch.tensor([1.0, 1.0, -0.3])
    v[::7, 2] = 0.02                                                         # in front of znear = 0.05
    faces = torch.arange(180).reshape(60, 3)
    c2w = torch.eye(4)[None]
    cam = mesh.Pinhole(torch.tensor([[0.9, 0.05, 0.5], [0.0, 0.9, 0.45], [0.0, 0.0, 1.0]]))
    proj = mesh.project(v, c2w, cam, (40, 44))
    assert proj.dropped.any() and not proj.dropped.all()
    fid, dep = mesh.rasterize(proj, faces, (40, 44))
    bfid, bdep, _ = brute_raster(proj.packed[0], faces, 40, 44, False)
    assert torch.equal(fid[0], bfid) and torch.equal(dep[0], bdep.to(torch.float32))
    hit = fid[0][fid[0] >= 0].long()
    assert not proj.dropped[0][faces[hit]].any()


def grid_mesh(seed, h, w, n=9):
    """A grid of (n + 1)^2 shared vertices covering more than the viewport, every cell split along a random diagonal with a random
    winding, faces shuffled.  Lattice points snap to pixel centres, some are jittered."""
    g = torch.Generator().manual_seed(seed)
    xs = torch.linspace(-2 * 256, (w + 2) * 256, n + 1).round().long()
    ys = torch.linspace(-2 * 256, (h + 2) * 256, n + 1).round().long()
    X, Y = torch.meshgrid(xs, ys, indexing='xy')
    X = (X >> 8 << 8) + 128
    Y = (Y >> 8 << 8) + 128
    jit = torch.rand(X.shape, generator=g) < 0.5
    inner = torch.zeros_like(jit)
    inner[1:-1, 1:-1] = True
    X = torch.where(jit & inner, X + torch.randint(-90, 90, X.shape, generator=g), X)
    Y = torch.where(jit & inner, Y + torch.randint(-90, 90, Y.shape, generator=g), Y)
    nv = (n + 1) ** 2
    packed = torch.stack([X.reshape(-1).int(), Y.reshape(-1).int(), torch.full([nv], 1.0).view(torch.int32), torch.zeros(nv, dtype=torch.int32)], -1)
    faces = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, i * (n + 1) + j + 1, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1
            tris = [[a, b, d], [a, d, c]] if torch.rand([], generator=g) < 0.5 else [[a, b, c], [b, d, c]]
            for t in tris:
                faces.append(t if torch.rand([], generator=g) < 0.5 else [t[0], t[2], t[1]])
    faces = torch.tensor(faces)
    return packed, faces[torch.randperm(len(faces), generator=g)]


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_fill_rule_covers_every_pixel_centre_once(seed):
    h, w = 36, 32
    packed, faces = grid_mesh(seed, h, w)
    _, _, count = brute_raster(packed, faces, h, w, True)
    assert (count == 1).all(), f'holes {(count == 0).sum()}, double hits {(count > 1).sum()}'
    fid, _ = mesh.rasterize(mesh.Projection(packed[None], True), faces, (h, w))
    assert (fid >= 0).all()


def test_pinhole_projects_ray_sampler_pixels_to_their_centres():
    from pix2pix3d_amd import configs
    from pix2pix3d_amd.training.volumetric_rendering.ray_sampler import RaySampler
    label = torch.tensor(np.stack([configs.orbit_camera(k, radius=2.7, focal=4.2647, pivot=(0, 0, 0.2)) for k in (3, 40)]))
    label[1, 16 + 1] = 0.07                                                  # a skewed camera as well
    c2w, K = label[:, :16].reshape(-1, 4, 4), label[:, 16:25].reshape(-1, 3, 3)
    res = 24
    origins, dirs = RaySampler()(c2w, K, res)
    for f in range(2):
        t = torch.linspace(2.3, 3.2, res * res)[:, None]
        pts = origins[f] + t * dirs[f]
        proj = mesh.project(pts, c2w[f:f + 1], mesh.Pinhole(K[f]), res)
        rows, cols = torch.meshgrid(torch.arange(res), torch.arange(res), indexing='ij')
        expect = torch.stack([cols.reshape(-1) * 256 + 128, rows.reshape(-1) * 256 + 128], -1)
        assert not proj.dropped.any()
        assert (proj.xy[0].long() - expect).abs().max() <= 1


def test_orthographic_roll_rotates_the_image():
    u = sphere(40, 14.0, centre=[18.3, 21.1, 19.7]) + torch.linspace(0, 3, 40)[:, None, None]   # a lopsided blob
    v, f = shape.marching_cubes(u, 0.0)
    v = v / 39 - 0.5
    g = torch.Generator().manual_seed(3)
    colors = torch.randint(0, 256, [len(v), 3], generator=g, dtype=torch.uint8)
    c2w = mesh.turntable_poses([0, 0, 0], 1.0, 1)[0]
    roll = torch.eye(4)
    roll[:3, 0], roll[:3, 1] = c2w[:3, 1], -c2w[:3, 0]                      # new right = old down, new down = -old right
    roll[:3, 2], roll[:3, 3] = c2w[:3, 2], c2w[:3, 3]
    cam = mesh.Orthographic(0.6, 0.6)
    a, fa, _ = mesh.render(v, f, c2w[None], cam, 64, colors=colors, return_buffers=True)
    b, fb, _ = mesh.render(v, f, roll[None], cam, 64, colors=colors, return_buffers=True)
    assert (fa >= 0).sum() > 500
    rot = torch.rot90(fa[0], 1, (0, 1))
    assert (rot != fb[0]).float().mean() < 2e-3                                # pixel centres exactly on an edge may change owner
    assert (torch.rot90(fa[0], -1, (0, 1)) != fb[0]).float().mean() > 0.05
    same = rot == fb[0]
    assert torch.equal(torch.rot90(a[0], 1, (0, 1))[same], b[0][same])


def _quad(tilt_deg, colour):
    t = math.radians(tilt_deg)
    corners = torch.tensor([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]]) * 0.4
    v = torch.stack([corners[:, 0], corners[:, 1] * math.cos(t), 2.0 + corners[:, 1] * math.sin(t)], -1)
    faces = torch.tensor([[0, 1, 2], [0, 3, 2]])                             # opposite windings: both sides render
    colors = torch.tensor([colour] * 4, dtype=torch.uint8)
    return v, faces, colors


@pytest.mark.parametrize('camera', [mesh.Orthographic(0.5, 0.5), mesh.Pinhole(torch.tensor([[1.6, 0, 0.5], [0, 1.6, 0.5], [0, 0, 1]]))])
def test_shading_flat_and_tilted_quad(camera):
    colour = (100, 40, 220)
    c2w = torch.eye(4)[None]
    v, f, c = _quad(0, colour)
    img, fid, _ = mesh.render(v, f, c2w, camera, 32, colors=c, background=(1, 2, 3), return_buffers=True)
    inside = fid[0] >= 0
    assert inside.sum() > 100 and (~inside).sum() > 0
    assert (img[0][inside] == torch.tensor(colour, dtype=torch.uint8)).all()
    assert (img[0][~inside] == torch.tensor([1, 2, 3], dtype=torch.uint8)).all()
    v, f, c = _quad(60, colour)
    img, fid, _ = mesh.render(v, f, c2w, camera, 32, colors=c, return_buffers=True)
    inside = fid[0] >= 0
    assert inside.sum() > 50
    amb = 0.3
    expect = torch.tensor([math.floor(k * (amb + (1 - amb) * 0.5) + 0.5) for k in colour], dtype=torch.uint8)
    assert (img[0][inside] == expect).all()
    grey = mesh.render(v, f, c2w, camera, 32)[0]
    assert (grey[inside] == math.floor(mesh.GREY * 0.65 + 0.5)).all()


def _look_at_pose_sampler(h, v, lookat, radius):
    """camera_utils.LookAtPoseSampler.sample with zero stddev, restated in float32 torch."""
    v = torch.clamp(torch.tensor([[v]], dtype=torch.float32), 1e-5, math.pi - 1e-5)
    theta = torch.tensor([[h]], dtype=torch.float32)
    phi = torch.arccos(1 - 2 * (v / math.pi))
    o = torch.zeros([1, 3])
    o[:, 0:1] = radius * torch.sin(phi) * torch.cos(math.pi - theta)
    o[:, 2:3] = radius * torch.sin(phi) * torch.sin(math.pi - theta)
    o[:, 1:2] = radius * torch.cos(phi)
    fwd = torch.nn.functional.normalize(lookat - o, dim=-1)
    up = torch.tensor([[0.0, 1.0, 0.0]])
    right = -torch.nn.functional.normalize(torch.cross(up, fwd, dim=-1), dim=-1)
    up = torch.nn.functional.normalize(torch.cross(fwd, right, dim=-1), dim=-1)
    m = torch.eye(4)
    m[:3, :3] = torch.stack([right[0], up[0], fwd[0]], -1)
    m[:3, 3] = o[0]
    return m


@pytest.mark.parametrize('cfg', ['cat', 'car'])
def test_turntable_equals_look_at_pose_sampler(cfg):
    n = 120
    if cfg == 'cat':
        pivot, radius, yaw0, yr, pr = [0, 0, -0.06], 1.0, 3.14 / 2, 0.35, 0.25
        poses = mesh.turntable_poses(pivot, radius, n)
    else:
        pivot, radius, yaw0, yr, pr = [0, 0, 0], 1.2, -3.14 / 2, np.pi, np.pi / 2
        poses = mesh.turntable_poses(pivot, radius, n, yaw0=yaw0, yaw_range=yr, pitch_range=pr)
    assert poses.shape == (n, 4, 4) and poses.dtype == torch.float32
    for k in range(n):
        ref = _look_at_pose_sampler(yaw0 + yr * np.sin(2 * 3.14 * k / n), 3.14 / 2 - 0.05 + pr * np.cos(2 * 3.14 * k / n),
                                    torch.tensor(pivot, dtype=torch.float32), radius)
        assert torch.allclose(poses[k], ref, atol=1e-4, rtol=0), (k, poses[k], ref)


def _parse_ply(path):
    data = open(path, 'rb').read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    header = data[:end].decode('ascii').split('\n')
    assert header[0] == 'ply' and header[1] == 'format binary_little_endian 1.0'
    nv = int([l for l in header if l.startswith('element vertex')][0].split()[-1])
    nf = int([l for l in header if l.startswith('element face')][0].split()[-1])
    has_colour = 'property uchar red' in header
    vdt = [('p', '<f4', (3,))] + ([('c', 'u1', (3,))] if has_colour else [])
    vrec = np.frombuffer(data, dtype=vdt, count=nv, offset=end)
    frec = np.frombuffer(data, dtype=[('n', 'u1'), ('i', '<i4', (3,))], count=nf, offset=end + vrec.nbytes)
    assert (frec['n'] == 3).all()
    return vrec['p'], frec['i'], (vrec['c'] if has_colour else None), end + vrec.nbytes + frec.nbytes, len(data)


@pytest.mark.parametrize('with_colour', [True, False])
def test_write_ply_round_trip(tmp_path, with_colour):
    v, f = shape.marching_cubes(sphere(20, 7.0), 0.0)
    colors = torch.randint(0, 256, [len(v), 3], generator=torch.Generator().manual_seed(0), dtype=torch.uint8) if with_colour else None
    path = tmp_path / 'm.ply'
    mesh.write_ply(path, v, f, colors)
    pv, pf, pc, expect_size, size = _parse_ply(path)
    assert size == expect_size
    assert np.array_equal(pv, v.numpy()) and np.array_equal(pf, f.numpy())
    if with_colour:
        assert np.array_equal(pc, colors.numpy())
    else:
        assert pc is None


def test_save_gif(tmp_path):
    from PIL import Image
    frames = torch.randint(0, 256, [5, 24, 32, 3], generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    path = tmp_path / 'a.gif'
    mesh.save_gif(path, frames, fps=60)
    im = Image.open(path)
    assert im.n_frames == 5 and im.size == (32, 24)


def test_closed_sphere_has_no_holes():
    n, r = 48, 17.0
    centre = [(n - 1) / 2 + 0.17, (n - 1) / 2 - 0.23, (n - 1) / 2 + 0.05]
    v, f = shape.marching_cubes(sphere(n, r, centre), 0.0)
    scale = 1.0 / (n - 1)
    v = v * scale - 0.5
    c_world = torch.tensor(centre) * scale - 0.5
    poses = mesh.turntable_poses([0, 0, 0], 1.0, 8, yaw_range=1.2, pitch_range=0.6)
    res, xmag = 96, 0.4
    fid = mesh.render(v, f, poses, mesh.Orthographic(xmag, xmag), res, return_buffers=True)[1]
    r_px = r * scale / xmag * res / 2
    for k in range(8):
        c2w = poses[k].double()
        cam = c2w[:3, :3].T @ (c_world.double() - c2w[:3, 3])
        cx, cy = (cam[0] / xmag + 1) / 2 * res, (cam[1] / xmag + 1) / 2 * res
        rows, cols = torch.meshgrid(torch.arange(res) + 0.5, torch.arange(res) + 0.5, indexing='ij')
        disc = (cols - cx) ** 2 + (rows - cy) ** 2 < (r_px - 1) ** 2
        assert disc.sum() > 1000
        assert (fid[k][disc] >= 0).all(), f'pose {k}: {(fid[k][disc] < 0).sum()} background pixels inside the disc'


@pytest.mark.parametrize('znear,zfar', [(0.0, 100.0), (-0.1, 100.0), (1.0, 1.0), (0.05, math.inf)])
def test_cameras_need_positive_znear_below_zfar(znear, zfar):
    v = torch.zeros([3, 3])
    for cam in (mesh.Orthographic(0.3, 0.3, znear, zfar), mesh.Pinhole(torch.eye(3), znear, zfar)):
        with pytest.raises(ValueError, match='znear'):
            mesh.project(v, torch.eye(4)[None], cam, 16)
    with pytest.raises(ValueError, match='xmag'):
        mesh.project(v, torch.eye(4)[None], mesh.Orthographic(0.0, 0.3), 16)


def test_shade_checks_its_buffers_agree():
    v, f = shape.marching_cubes(sphere(20, 7.0), 0.0)
    v = v / 19 - 0.5
    poses = mesh.turntable_poses([0, 0, 0], 1.0, 2)
    proj = mesh.project(v, poses, mesh.Orthographic(0.6, 0.6), 32)
    fid, _ = mesh.rasterize(proj, f, 32)
    with pytest.raises(ValueError, match='projection'):
        mesh.shade(fid, proj, v[:-1], f, poses)
    with pytest.raises(ValueError, match='projection'):
        mesh.shade(fid[:1], proj, v, f, poses[:1])
    with pytest.raises(ValueError, match='cameras'):
        mesh.shade(fid, proj, v, f, poses[:1])
    assert mesh.shade(fid, proj, v, f, poses).shape == (2, 32, 32, 3)


class _FakeGenerator:
    """Just what extract_mesh reads: rendering_kwargs, data_type, semantic_channels and sample_mixed (label logits x, y, then zeros)."""
    def __init__(self, data_type, semantic_channels):
        self.rendering_kwargs = {'avg_camera_pivot': [0, 0, 0], 'box_warp': 1.0}
        self.data_type, self.semantic_channels = data_type, semantic_channels

    def sample_mixed(self, pts, directions, ws, truncation_psi=1, noise_mode='const'):
        rgb = torch.zeros([1, pts.shape[1], 32 + self.semantic_channels])
        rgb[0, :, 32] = pts[0, :, 0]
        if self.semantic_channels > 1:
            rgb[0, :, 33] = pts[0, :, 1]
        return {'rgb': rgb}


@pytest.mark.parametrize('data_type,channels,labelled,xmag', [(None, 6, True, 0.3), ('seg', 6, True, 0.3), ('edge', 1, False, 0.6),
                                                               (None, 1, False, 0.3)])
def test_extract_mesh_chooses_the_scripts_branch(monkeypatch, data_type, channels, labelled, xmag):
    v, f = shape.marching_cubes(sphere(20, 7.0), 0.0)
    v = v / 19 - 0.5
    monkeypatch.setattr(shape, 'extract_geometry', lambda G, ws, resolution, threshold, **kw: (v, f))
    seen = {}
    real_render = mesh.render

    def spy(vertices, faces, poses, camera, size, colors=None):
        seen['camera'], seen['poses'] = camera, poses
        return real_render(vertices, faces, poses, camera, size, colors=colors)
    monkeypatch.setattr(mesh, 'render', spy)
    G = _FakeGenerator(data_type, channels)
    _, _, colors, frames = mesh.extract_mesh(G, torch.zeros([1, 1, 1]), resolution=20, threshold=0.0, n_frames=2, image_size=32)
    assert frames.shape == (2, 32, 32, 3)
    assert seen['camera'] == mesh.Orthographic(xmag, xmag)
    radius = 1.0 if xmag == 0.3 else 1.2
    assert torch.allclose(seen['poses'][:, :3, 3].norm(dim=-1), torch.tensor(radius))
    if labelled:
        sem = torch.zeros([len(v), channels])
        sem[:, 0], sem[:, 1] = v[:, 0], v[:, 1]
        labels = sem.argmax(-1)
        assert len(labels.unique()) > 2
        assert torch.equal(colors, mesh.default_palette(channels)[labels])
    else:
        assert colors is None


# ---- view groups ------------------------------------------------------------------------------------------------------------------
def grouped_views():
    """(vertices, faces, colours, poses [3, 4, 4], camera) of test_texture_host.py's two spheres: three pinhole views, each with a focal
    length of its own, so that a group of views that took another frame's intrinsics would show."""
    from test_texture_host import camera_kinds, two_sphere_scene
    v, f, colors = two_sphere_scene()
    poses, cam = camera_kinds(2.2)['pinhole']
    k = cam.intrinsics.repeat(3, 1, 1)
    k[:, 0, 0] = k[:, 1, 1] = torch.tensor([2.0, 2.2, 2.5])
    return v, f, colors, poses[:3], mesh.Pinhole(k)


def check_view_groups(render, n_points, frame_of):
    """``render(poses, camera, **kw)`` with one view per group and with groups of two gives the bytes of the single default group,
    frames and buffers; ``frame_of(k)`` is frame k rendered alone with its own intrinsics."""
    _, _, _, poses, cam = grouped_views()
    whole = render(poses, cam, return_buffers=True)
    assert len(whole) == 3 and all(len(t) == 3 for t in whole) and (whole[1] >= 0).sum() > 1000
    for max_bytes in (1, 2 * 16 * n_points):
        part = render(poses, cam, return_buffers=True, max_bytes=max_bytes)
        for a, b, what in zip(part, whole, ('frames', 'face_id', 'depth')):
            assert a.dtype == b.dtype and torch.equal(a, b), (max_bytes, what)
        assert torch.equal(render(poses, cam, max_bytes=max_bytes), whole[0])
    for k in range(3):
        assert torch.equal(frame_of(k)[0], whole[0][k])
    assert not torch.equal(render(poses[2:], mesh.Pinhole(cam.intrinsics[0]))[0], whole[0][2])       # the focal length shows
    with pytest.raises((ValueError, RuntimeError)):                      # two sets of intrinsics for three frames
        render(poses, mesh.Pinhole(cam.intrinsics[:2]))


def test_render_in_groups_of_views_gives_the_bytes_of_one_group():
    v, f, colors, poses, cam = grouped_views()

    def render(poses, camera, **kw):
        return mesh.render(v, f, poses, camera, 96, colors=colors, **kw)
    check_view_groups(render, len(v), lambda k: render(poses[k:k + 1], mesh.Pinhole(cam.intrinsics[k])))


def test_render_names_an_intrinsics_count_that_fits_no_frame_count():
    v, f, _, poses, cam = grouped_views()
    with pytest.raises(ValueError, match='render: 2 intrinsics for 3 frames'):
        mesh.render(v, f, poses, mesh.Pinhole(cam.intrinsics[:2]), 96)
