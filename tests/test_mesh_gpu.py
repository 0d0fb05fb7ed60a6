"""pix2pix3d_amd.mesh on the device: p3d_mesh_project, the tiled rasterizer and p3d_mesh_shade against the CPU path (the rasterizer
bit for bit on identical projected inputs), determinism and face-order independence, extract_mesh on the seeded generators, and a
120-frame 512^2 turntable of a mesh with millions of faces."""
import numpy as np
import pytest
import torch

from model_cases import build_generator
from pix2pix3d_amd import _lib, mesh, shape
from test_mesh_host import grid_mesh, random_soup
from test_shape_host import sphere

pytestmark = pytest.mark.gpu


def _cameras(kind):
    if kind == 'ortho':
        return mesh.turntable_poses([0, 0, -0.06], 1.0, 4), mesh.Orthographic(0.3, 0.3)
    from pix2pix3d_amd import configs
    labels = torch.tensor(np.stack([configs.orbit_camera(k, radius=2.7, pivot=(0, 0, 0.2)) for k in (0, 17, 33, 90)]))
    return labels[:, :16].reshape(-1, 4, 4), mesh.Pinhole(labels[:, 16:25].reshape(-1, 3, 3))


def _bumpy_sphere(n, r, amp=2.5, period=5.0):
    g = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float32)] * 3, indexing='ij'), -1)
    bump = amp * torch.sin(g[..., 0] / period) * torch.sin(g[..., 1] / period) * torch.sin(g[..., 2] / period)
    return sphere(n, r) + bump


def _gyroid_ball(n, r, period):
    """A ball filled with a gyroid: millions of small faces at n = 256."""
    g = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float32)] * 3, indexing='ij'), -1) / period
    x, y, z = g.unbind(-1)
    gyroid = torch.sin(x) * torch.cos(y) + torch.sin(y) * torch.cos(z) + torch.sin(z) * torch.cos(x)
    return torch.minimum(sphere(n, r), gyroid * period)


def _mc_mesh(u):
    v, f = shape.marching_cubes(u.cuda(), 0.0)
    return (v / (u.shape[0] - 1) - 0.5).cpu(), f.cpu()


def _check_raster(proj, faces, res):
    """Device raster on the CPU projection, against the CPU raster: face id and depth bit for bit."""
    n0 = _lib.launch_count('aux')
    fid, dep = mesh.rasterize(proj.to('cuda'), faces.cuda(), res)
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') >= n0 + 3
    cfid, cdep = mesh.rasterize(proj, faces, res)
    assert torch.equal(fid.cpu(), cfid)
    assert torch.equal(dep.cpu(), cdep)
    return cfid, cdep


@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
def test_project_matches_cpu(hip_lib, kind):
    g = torch.Generator().manual_seed(1)
    v = (torch.rand([50_000, 3], generator=g) - 0.5) * 1.2
    v[:100] *= 400                                                           # beyond the guard band / behind the camera
    c2w, cam = _cameras(kind)
    p_dev = mesh.project(v.cuda(), c2w, cam, (512, 480))
    p_cpu = mesh.project(v, c2w, cam, (512, 480))
    assert p_dev.packed.shape == (4, 50_000, 4)
    assert torch.equal(p_dev.dropped.cpu(), p_cpu.dropped)
    assert p_cpu.dropped.any() and not p_cpu.dropped.all()
    assert (p_dev.xy.cpu().long() - p_cpu.xy.long()).abs().max() <= 1
    z_dev, z_cpu = p_dev.z.cpu(), p_cpu.z
    assert ((z_dev - z_cpu).abs() <= 1e-6 * z_cpu.abs()).all()


@pytest.mark.parametrize('seed,size', [(0, (96, 160)), (1, (257, 200)), (2, (512, 512))])
@pytest.mark.parametrize('ortho', [True, False])
def test_raster_random_soups(hip_lib, seed, size, ortho):
    h, w = size
    packed, faces = random_soup(seed, h, w, n=3000)
    _check_raster(mesh.Projection(packed[None], ortho), faces, size)


def test_raster_full_screen_triangles(hip_lib):
    """Triangles reaching into the guard band on every side: each crosses every tile of a 512^2 image; depth ties between them."""
    h = w = 512
    g = torch.Generator().manual_seed(4)
    lo, hi = -4000 * 256, (512 + 4000) * 256
    x = torch.randint(lo, hi, [24], generator=g)
    y = torch.randint(lo, hi, [24], generator=g)
    x[:3] = torch.tensor([lo, hi, lo])
    y[:3] = torch.tensor([lo, lo, hi])
    x[3:6] = torch.tensor([hi, lo, hi])
    y[3:6] = torch.tensor([hi, hi, lo])
    z = torch.rand([24], generator=g) + 1.0
    z[:6] = 1.5
    packed = torch.stack([x.int(), y.int(), z.view(torch.int32), torch.zeros(24, dtype=torch.int32)], -1)
    faces = torch.arange(24).reshape(8, 3)
    for ortho in (True, False):
        fid, _ = _check_raster(mesh.Projection(packed[None].repeat(2, 1, 1), ortho), faces, (h, w))
        assert (fid >= 0).all()
    gp, gf = grid_mesh(0, 512, 512, n=5)                                     # a coarse grid of big triangles: every pixel once
    fid, _ = _check_raster(mesh.Projection(gp[None], True), gf, (512, 512))
    assert (fid >= 0).all()


@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
def test_raster_sphere_128(hip_lib, kind):
    v, f = _mc_mesh(sphere(128, 50.0))
    assert len(f) > 50_000
    c2w, cam = _cameras(kind)
    if kind == 'pinhole':
        v = v * 0.5
    proj = mesh.project(v, c2w, cam, 256)
    fid, _ = _check_raster(proj, f, 256)
    assert ((fid >= 0).sum(dim=(1, 2)) > 1000).all()


def test_raster_gyroid_ball_256_eight_frames(hip_lib):
    v, f = _mc_mesh(_gyroid_ball(256, 100.0, 2.5))
    assert len(f) > 2_000_000
    poses = mesh.turntable_poses([0, 0, 0], 1.0, 8, yaw_range=1.5, pitch_range=0.8)
    proj = mesh.project(v, poses, mesh.Orthographic(0.5, 0.5), 512)
    fid, _ = _check_raster(proj, f, 512)
    assert ((fid >= 0).sum(dim=(1, 2)) > 50_000).all()


def _median_mesh(name, resolution):
    G = build_generator(name, 'cuda')
    ws = torch.randn([1, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(0)).cuda()
    thr = float(shape.sigma_grid(G, ws, resolution)[0].median())
    return G, ws, thr


def test_raster_seg2cat_mesh_256(hip_lib):
    G, ws, thr = _median_mesh('seg2cat', 256)
    v, f = shape.extract_geometry(G, ws, 256, thr)
    assert len(f) > 1_000_000
    poses = mesh.turntable_poses(G.rendering_kwargs['avg_camera_pivot'], 1.0, 4)
    proj = mesh.project(v.cpu(), poses, mesh.Orthographic(0.3, 0.3), 512)
    fid, _ = _check_raster(proj, f.cpu(), 512)
    assert ((fid >= 0).sum(dim=(1, 2)) > 10_000).all()


def test_raster_deterministic_and_order_independent(hip_lib):
    v, f = _mc_mesh(_bumpy_sphere(128, 50.0, amp=2.0, period=3.0))
    poses = mesh.turntable_poses([0, 0, 0], 1.0, 3)
    proj = mesh.project(v.cuda(), poses, mesh.Orthographic(0.5, 0.5), 384)
    fc = f.cuda()
    a = mesh.rasterize(proj, fc, 384)
    b = mesh.rasterize(proj, fc, 384)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    perm = torch.arange(len(f) - 1, -1, -1, device='cuda')
    r = mesh.rasterize(proj, fc[perm], 384)
    assert torch.equal(r[1], a[1])                                          # the nearest depth does not depend on the order
    hit = r[0] >= 0
    assert torch.equal(hit, a[0] >= 0)
    back = torch.where(hit, perm[r[0].long().clamp(min=0)], torch.full_like(perm[:1], -1)).to(torch.int32)
    differ = back != a[0]
    assert differ.float().mean() < 1e-3
    # every pixel where they differ is a depth tie: both faces cover its centre at exactly the nearest depth, and each run kept the
    # lower of its own ids (the forward run the lower original id)
    k, row, col = differ.nonzero().cpu().unbind(1)
    fa, fb = a[0][differ].long().cpu(), back[differ].long().cpu()
    assert (fa < fb).all()
    packed = proj.packed.cpu()
    nearest = a[1][differ].cpu()
    for ids in (fa, fb):
        for frame in k.unique().tolist():
            m = k == frame
            ok, _, x, y, z = mesh._setup_cpu(packed[frame], f[ids[m]])
            w0, w1, w2, inside = mesh._weights(x, y, row[m], col[m])
            assert (ok & inside).all()
            assert torch.equal(mesh._depth(w0, w1, w2, z, True), nearest[m])


def test_shade_moves_inputs_to_the_face_id_device(hip_lib):
    """CPU vertices, colours and projection with a device face_id: shade moves them (no host pointer reaches the kernel)."""
    v, f = _mc_mesh(sphere(64, 25.0))
    poses = mesh.turntable_poses([0, 0, 0], 1.0, 2)
    proj = mesh.project(v, poses, mesh.Orthographic(0.6, 0.6), 128)
    fid, _ = mesh.rasterize(proj, f, 128)
    colors = torch.randint(0, 256, [len(v), 3], generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    mixed = mesh.shade(fid.cuda(), proj, v, f, poses, colors)
    same = mesh.shade(fid.cuda(), proj.to('cuda'), v.cuda(), f.cuda(), poses, colors.cuda())
    assert mixed.is_cuda and torch.equal(mixed, same)
    assert torch.equal(mixed.cpu(), mesh.shade(fid, proj.to('cuda'), v.cuda(), f, poses, colors.cuda()))


@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
@pytest.mark.parametrize('with_colour', [True, False])
def test_shade_matches_cpu(hip_lib, kind, with_colour):
    v, f = _mc_mesh(_bumpy_sphere(96, 38.0, amp=1.5, period=4.0))
    c2w, cam = _cameras(kind)
    if kind == 'pinhole':
        v = v * 0.5
    colors = torch.randint(0, 256, [len(v), 3], generator=torch.Generator().manual_seed(2), dtype=torch.uint8) if with_colour else None
    proj = mesh.project(v, c2w, cam, 300)
    fid, _ = mesh.rasterize(proj, f, 300)
    cpu = mesh.shade(fid, proj, v, f, c2w, colors, background=(10, 255, 0), ambient=0.25)
    n0 = _lib.launch_count('aux')
    dev = mesh.shade(fid.cuda(), proj.to('cuda'), v.cuda(), f.cuda(), c2w, None if colors is None else colors.cuda(),
                     background=(10, 255, 0), ambient=0.25)
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') > n0
    assert (dev.cpu().int() - cpu.int()).abs().max() <= 1
    assert (fid >= 0).sum() > 10_000


@pytest.mark.parametrize('name', ['seg2cat', 'edge2car'])
def test_extract_mesh_equals_cpu_render(hip_lib, name):
    G, ws, thr = _median_mesh(name, 128)
    n0 = _lib.launch_count('aux')
    v, f, colors, frames = mesh.extract_mesh(G, ws, resolution=128, threshold=thr, n_frames=8)
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') > n0
    assert frames.shape == (8, 512, 512, 3) and frames.is_cuda and frames.dtype == torch.uint8
    if name == 'seg2cat':
        labels, col2 = mesh.vertex_labels(G, ws, v)
        with torch.no_grad():
            sem = G.sample_mixed(v[None], None, ws, noise_mode='const')['rgb'][0, :, 32:32 + G.semantic_channels]
        assert torch.equal(labels, sem.argmax(-1))
        assert torch.equal(colors, mesh.default_palette(G.semantic_channels).cuda()[labels]) and torch.equal(col2, colors)
        assert len(labels.unique()) > 1
        poses, cam = mesh.turntable_poses(G.rendering_kwargs['avg_camera_pivot'], 1.0, 8), mesh.Orthographic(0.3, 0.3)
    else:
        assert colors is None
        poses = mesh.turntable_poses(G.rendering_kwargs['avg_camera_pivot'], 1.2, 8, yaw0=-3.14 / 2, yaw_range=np.pi, pitch_range=np.pi / 2)
        cam = mesh.Orthographic(0.6, 0.6)
    ref = mesh.render(v.cpu(), f.cpu(), poses, cam, 512, colors=None if colors is None else colors.cpu())
    assert (frames.cpu().int() - ref.int()).abs().max() <= 1
    background = (frames.cpu() == 255).all(-1)
    assert ((~background).sum(dim=(1, 2)) > 500).all()


def test_turntable_120_frames_large_mesh(hip_lib):
    G, ws, thr = _median_mesh('seg2cat', 512)
    v, f = shape.extract_geometry(G, ws, 512, thr)
    assert len(f) >= 5_000_000
    poses = mesh.turntable_poses(G.rendering_kwargs['avg_camera_pivot'], 1.0, 120)
    cam = mesh.Orthographic(0.3, 0.3)
    frames, fid, _ = mesh.render(v, f, poses, cam, 512, return_buffers=True)
    torch.cuda.synchronize()
    assert frames.shape == (120, 512, 512, 3)
    assert ((fid >= 0).sum(dim=(1, 2)) > 10_000).all()
    fc = f.cpu()
    for k in (0, 60):
        proj = mesh.project(v, poses[k:k + 1], cam, 512).to('cpu')           # the projection render made, on identical inputs
        ref, _ = mesh.rasterize(proj, fc, 512)
        assert torch.equal(fid[k:k + 1].cpu(), ref)
