"""pix2pix3d_amd.mesh filtering on the device: p3d_mesh_smooth_step and p3d_mesh_label_vote against the CPU formulation bit for bit
(closed and open meshes, many work-groups, the hub of a fan with a list of 50 000), p3d_mesh_shade_smooth against the CPU shade,
determinism and face-order independence, and the filters inside extract_mesh, textured_mesh and atlas_mesh on the seeded generators."""
import functools

import pytest
import torch

from conftest import record_error
from pix2pix3d_amd import _lib, atlas, mesh, texture
from test_mesh_cleanup_host import fan, three_spheres
from test_mesh_filter_host import open_sphere
from test_mesh_gpu import _bumpy_sphere, _cameras, _gyroid_ball, _mc_mesh, _median_mesh

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name):
    """(vertices float32 [V, 3], faces int64 [T, 3]) on the CPU.  Do not modify."""
    if name == 'three_spheres':
        return three_spheres()
    if name == 'open_sphere':
        return open_sphere()
    if name == 'gyroid':
        v, f = _mc_mesh(_gyroid_ball(96, 38.0, 2.5))
        assert len(v) > 50_000                                              # hundreds of work-groups
        return v, f
    faces, nv = fan(50_000)
    return torch.rand([nv, 3], generator=torch.Generator().manual_seed(7)), faces


def _worst_ulp(a, b):
    """The largest distance in units of the last place between two float32 tensors of one sign pattern (0 = the same bits)."""
    return int((a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs().max())


def _assert_same_floats(name, dev, cpu):
    assert dev.is_cuda and dev.dtype == torch.float32 and dev.shape == cpu.shape
    ulp = _worst_ulp(dev.cpu(), cpu)
    record_error(name, ulp)
    print(f'{name}: worst ulp {ulp}')
    assert ulp == 0 and torch.equal(dev.cpu().view(torch.int32), cpu.view(torch.int32))


@pytest.mark.parametrize('name', ['three_spheres', 'open_sphere', 'gyroid', 'fan'])
def test_smooth_matches_cpu(hip_lib, name):
    v, f = _case(name)
    pin = name != 'fan'                                                     # the fan's ring is all boundary: free it so that everything moves
    cpu = mesh.smooth(v, f, iterations=2, pin_boundary=pin)
    n0 = _lib.launch_count('aux')
    dev = mesh.smooth(v.cuda(), f.cuda(), iterations=2, pin_boundary=pin)
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') == n0 + 4                               # one launch per step
    _assert_same_floats(f'mesh_smooth_ulp_{name}', dev, cpu)
    assert not torch.equal(cpu, v)
    one = mesh.smooth(v.cuda(), f.cuda(), iterations=1, lam=0.8, mu=0, pin_boundary=False)      # a single smooth_step
    _assert_same_floats(f'mesh_smooth_step_ulp_{name}', one, mesh.smooth(v, f, iterations=1, lam=0.8, mu=0, pin_boundary=False))


@pytest.mark.parametrize('channels', [1, 7, 64])
def test_smooth_values_matches_cpu(hip_lib, channels):
    v, f = _case('three_spheres')
    g = torch.Generator().manual_seed(channels)
    x = torch.randn([len(v), channels], generator=g) * 50
    pinned = torch.rand(len(v), generator=g) < 0.2
    adj = mesh.adjacency(f, len(v))
    n0 = _lib.launch_count('aux')
    dev = mesh.smooth_values(x.cuda(), f.cuda(), iterations=3, factor=0.6, pinned=pinned.cuda())
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') == n0 + 3
    _assert_same_floats(f'mesh_smooth_values_ulp_c{channels}', dev, mesh.smooth_values(x, f, iterations=3, factor=0.6, pinned=pinned, adjacency=adj))
    assert torch.equal(dev[pinned.cuda()].cpu(), x[pinned])
    colours = torch.randint(0, 256, [len(v), channels], generator=g, dtype=torch.uint8)
    got = mesh.smooth_values(colours.cuda(), f.cuda(), iterations=2, adjacency=adj)          # a CPU adjacency is moved
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), mesh.smooth_values(colours, f, iterations=2))


def test_smooth_step_rejects_overlapping_buffers(hip_lib):
    v, f = _case('three_spheres')
    adj = mesh.adjacency(f.cuda(), len(v))
    x = v.cuda().contiguous()
    n0 = _lib.launch_count('aux')
    call = lambda out: hip_lib.p3d_mesh_smooth_step(_lib.ptr(x), len(v), 3, _lib.ptr(adj.offsets), _lib.ptr(adj.neighbours),       # noqa: E731
                                                    adj.neighbours.shape[0], None, 0.5, _lib.ptr(out), _lib.stream_of(x))
    assert call(x) == -2 and b'overlaps' in hip_lib.p3d_last_error()
    assert call(x[1:]) == -2
    labels = torch.zeros([len(v)], dtype=torch.uint8, device='cuda')
    assert hip_lib.p3d_mesh_label_vote(_lib.ptr(labels), len(v), 6, _lib.ptr(adj.offsets), _lib.ptr(adj.neighbours), adj.neighbours.shape[0],
                                       None, _lib.ptr(labels), _lib.stream_of(labels)) == -2
    assert _lib.launch_count('aux') == n0                                   # nothing was launched
    out = torch.empty_like(x)
    assert call(out) == 0
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') == n0 + 1
    assert torch.equal(out.cpu().view(torch.int32), mesh.smooth(v, f, 1, 0.5, 0, pin_boundary=False).view(torch.int32))


@pytest.mark.parametrize('name,n_labels', [('three_spheres', 6), ('three_spheres', 256), ('open_sphere', 6), ('gyroid', 6), ('fan', 6)])
def test_smooth_labels_matches_cpu(hip_lib, name, n_labels):
    v, f = _case(name)
    g = torch.Generator().manual_seed(n_labels + len(v))
    labels = torch.randint(0, n_labels, [len(v)], generator=g)
    pinned = torch.rand(len(v), generator=g) < 0.1
    if name == 'fan':
        pinned[-1] = False                                                  # the hub votes: the work-group path
        assert int(mesh.adjacency(f, len(v)).offsets.diff().max()) == 50_000
    for iterations, pin in ((1, None), (3, pinned)):
        cpu = mesh.smooth_labels(labels, f, iterations, n_labels, pinned=pin)
        n0 = _lib.launch_count('aux')
        dev = mesh.smooth_labels(labels.cuda(), f.cuda(), iterations, n_labels, pinned=None if pin is None else pin.cuda())
        torch.cuda.synchronize()
        assert _lib.launch_count('aux') == n0 + iterations
        assert dev.is_cuda and dev.dtype == torch.int64 and torch.equal(dev.cpu(), cpu)
        assert not torch.equal(cpu, labels)
        if pin is not None:
            assert torch.equal(cpu[pin], labels[pin])


def test_label_vote_of_a_hub_follows_its_ring(hip_lib):
    """The hub of the fan counts 50 000 labels: label 3 on 30 000 of the ring and 1 on the rest; ties at the hub go to the smaller label."""
    f, nv = fan(50_000)
    labels = torch.full([nv], 1)
    labels[:30_000] = 3
    labels[-1] = 5
    n0 = _lib.launch_count('aux')
    out = mesh.smooth_labels(labels.cuda(), f.cuda(), n_labels=6)
    assert _lib.launch_count('aux') > n0
    assert int(out[-1]) == 3 and torch.equal(out.cpu(), mesh.smooth_labels(labels, f, n_labels=6))
    labels[:25_000], labels[25_000:-1] = 4, 2
    out = mesh.smooth_labels(labels.cuda(), f.cuda())
    assert int(out[-1]) == 2 and torch.equal(out.cpu(), mesh.smooth_labels(labels, f))
    labels[-1] = 4                                                          # 25 001 against 25 000: its own label wins
    assert int(mesh.smooth_labels(labels.cuda(), f.cuda())[-1]) == 4


@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
@pytest.mark.parametrize('with_colour', [True, False])
def test_shade_with_normals_matches_cpu(hip_lib, kind, with_colour):
    v, f = _mc_mesh(_bumpy_sphere(96, 38.0, amp=1.5, period=4.0))
    c2w, cam = _cameras(kind)
    if kind == 'pinhole':
        v = v * 0.5
    normals = texture.vertex_normals(v, f)
    colors = torch.randint(0, 256, [len(v), 3], generator=torch.Generator().manual_seed(2), dtype=torch.uint8) if with_colour else None
    proj = mesh.project(v, c2w, cam, 300)
    fid, _ = mesh.rasterize(proj, f, 300)
    cpu = mesh.shade(fid, proj, v, f, c2w, colors, background=(10, 255, 0), ambient=0.25, normals=normals)
    n0 = _lib.launch_count('aux')
    dev = mesh.shade(fid.cuda(), proj.to('cuda'), v.cuda(), f.cuda(), c2w, None if colors is None else colors.cuda(),
                     background=(10, 255, 0), ambient=0.25, normals=normals.cuda())
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') == n0 + 1
    worst = int((dev.cpu().int() - cpu.int()).abs().max())
    record_error(f'mesh_shade_smooth_bytes_{kind}_{int(with_colour)}', worst)
    assert worst <= 1
    assert (fid >= 0).sum() > 10_000
    flat = mesh.shade(fid.cuda(), proj.to('cuda'), v.cuda(), f.cuda(), c2w, None if colors is None else colors.cuda(),
                      background=(10, 255, 0), ambient=0.25)
    assert not torch.equal(flat, dev)


def test_filters_are_deterministic_and_order_independent(hip_lib):
    v, f = _case('gyroid')
    vc, fc = v.cuda(), f.cuda()
    labels = torch.randint(0, 6, [len(v)], generator=torch.Generator().manual_seed(9)).cuda()
    n0 = _lib.launch_count('aux')
    a, la = mesh.smooth(vc, fc, 3), mesh.smooth_labels(labels, fc, 2, 6)
    b, lb = mesh.smooth(vc, fc, 3), mesh.smooth_labels(labels, fc, 2, 6)
    back = fc.flip(0)[:, [1, 2, 0]].contiguous()
    c, lc = mesh.smooth(vc, back, 3), mesh.smooth_labels(labels, back, 2, 6)
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') == n0 + 3 * (6 + 2)
    for other in (b, c):
        assert torch.equal(a.view(torch.int32), other.view(torch.int32))
    assert torch.equal(la, lb) and torch.equal(la, lc)


@pytest.mark.parametrize('name', ['seg2cat', 'edge2car'])
def test_extract_mesh_with_the_filters(hip_lib, name):
    G, ws, thr = _median_mesh(name, 128)
    step = G.rendering_kwargs['box_warp'] / 127.0
    kw = dict(resolution=128, threshold=thr, n_frames=4, keep=1, cell=2 * step)
    v0, f0, colors0, frames0 = mesh.extract_mesh(G, ws, **kw)
    n0 = _lib.launch_count('aux')
    v, f, colors, frames = mesh.extract_mesh(G, ws, smooth=5, smooth_labels=2, smooth_shading=True, **kw)
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') > n0
    assert torch.equal(f, f0) and v.shape == v0.shape and not torch.equal(v, v0)
    assert torch.equal(v.view(torch.int32), mesh.smooth(v0, f0, 5).view(torch.int32))
    if name == 'seg2cat':
        labels = mesh.vertex_labels(G, ws, v0)[0]
        voted = mesh.smooth_labels(labels, f0, 2, n_labels=int(G.semantic_channels))
        assert torch.equal(colors, mesh.default_palette(int(G.semantic_channels)).cuda()[voted])
        assert torch.equal(voted.cpu(), mesh.smooth_labels(labels.cpu(), f0.cpu(), 2, n_labels=int(G.semantic_channels)))
    else:
        assert colors is None and colors0 is None
    assert frames.shape == frames0.shape and not torch.equal(frames, frames0)
    background = (frames == 255).all(-1)
    assert ((~background).sum(dim=(1, 2)) > 500).all()
    poses, cam = mesh.script_turntable(G, 4)
    ref = mesh.render(v.cpu(), f.cpu(), poses, cam, 512, colors=None if colors is None else colors.cpu(),
                      normals=texture.vertex_normals(v, f).cpu())
    assert (frames.cpu().int() - ref.int()).abs().max() <= 1


def test_textured_mesh_and_atlas_mesh_with_smoothing(hip_lib, tmp_path):
    G, ws, thr = _median_mesh('seg2cat', 128)
    step = G.rendering_kwargs['box_warp'] / 127.0
    kw = dict(resolution=128, threshold=thr, n_frames=2, image_size=128, keep=1, cell=2 * step, n_views=3)
    v0, f0 = mesh._clean_geometry(G, ws, 128, thr, 1, 1, 2 * step)
    want = mesh.smooth(v0, f0, 5)
    n0 = _lib.launch_count('aux')
    v, f, colors, seen, frames = texture.textured_mesh(G, ws, 'seg2cat', smooth=5, path=str(tmp_path / 'cat.ply'), **kw)
    assert _lib.launch_count('aux') > n0
    assert torch.equal(f, f0) and torch.equal(v.view(torch.int32), want.view(torch.int32)) and not torch.equal(v, v0)
    assert tuple(colors.shape) == (len(v), 3) and tuple(frames.shape) == (2, 128, 128, 3) and (seen > 0).any()
    assert (tmp_path / 'cat.ply').stat().st_size > len(v) * 27
    v, f, lay, tex, seen, frames = atlas.atlas_mesh(G, ws, 'seg2cat', size=2048, smooth=5, path=str(tmp_path / 'cat.obj'), **kw)
    assert torch.equal(v.view(torch.int32), want.view(torch.int32)) and torch.equal(f, atlas.orient_faces(want, f0))
    assert tuple(tex.shape) == (2048, 2048, 3) and tuple(frames.shape) == (2, 128, 128, 3) and (seen > 0).any()
    assert sorted(p.name for p in tmp_path.iterdir()) == ['cat.mtl', 'cat.obj', 'cat.ply', 'cat.png']
