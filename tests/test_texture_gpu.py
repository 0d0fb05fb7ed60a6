"""csrc/mesh_bake.hip against the CPU formulation of pix2pix3d_amd/texture.py (bit for bit on identical buffers), chaining of view groups
on the device, the whole textured_mesh pipeline and a large mesh."""
import pytest
import torch

from pix2pix3d_amd import _lib, mesh, texture, views
from test_mesh_gpu import _gyroid_ball, _mc_mesh, _median_mesh
from test_texture_host import camera_kinds, run_bake, soup_inputs, sphere_scene, true_colors, two_sphere_scene

pytestmark = pytest.mark.gpu

_buffers = {}


def _scene_buffers(name, kind):
    """(proj, face_id, depth, frames, vertices, normals, poses) of a scene on the CPU, computed once and left unchanged: both paths get
    these same buffers, so that only the new kernels are compared."""
    if (name, kind) not in _buffers:
        v, f, colors = sphere_scene() if name == 'sphere' else two_sphere_scene()
        focal, size = (4.2647, 128) if name == 'sphere' else (2.2, 96)
        poses, cam = camera_kinds(focal)[kind]
        proj = mesh.project(v, poses, cam, size)
        fid, dep = mesh.rasterize(proj, f, size)
        frames = mesh.shade(fid, proj, v, f, poses, colors, ambient=1.0)
        _buffers[name, kind] = (proj, fid, dep, frames, v, texture.vertex_normals(v, f), poses)
    return _buffers[name, kind]


def _parity(inputs, tolerance=0.01, power=2, min_cos=0.1, fallback=(200, 200, 200), groups=None):
    """Device bake == CPU bake on the same inputs: colours, seen and the fp64 sums themselves."""
    proj, fid, dep, frames, v, n, poses = inputs
    cpu = run_bake('cpu', proj, fid, dep, frames, v, n, poses, tolerance, power, min_cos, fallback)
    n0 = _lib.launch_count('aux')
    fb = fallback.cuda() if torch.is_tensor(fallback) else fallback
    dev = run_bake('cuda', proj.to('cuda'), fid.cuda(), dep.cuda(), frames.cuda(), v.cuda(), n.cuda(), poses, tolerance, power, min_cos, fb, groups)
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') >= n0 + 2
    assert dev[0].is_cuda and dev[0].dtype == torch.uint8 and dev[1].dtype == torch.int32
    assert torch.equal(dev[1].cpu(), cpu[1]), 'seen'
    assert torch.equal(dev[2].cpu(), cpu[2]), 'sums'
    assert torch.equal(dev[0].cpu(), cpu[0]), 'colours'
    return cpu


# ---- 8. parity with the CPU formulation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
@pytest.mark.parametrize('name', ['sphere', 'two'])
def test_bake_matches_cpu_on_the_sphere_scenes(hip_lib, name, kind):
    colors, seen, _ = _parity(_scene_buffers(name, kind))
    assert float((seen > 0).float().mean()) >= 0.98


@pytest.mark.parametrize('name', ['sphere', 'two'])
def test_vertex_normals_match_cpu(hip_lib, name):
    v, f, _ = sphere_scene() if name == 'sphere' else two_sphere_scene()
    n0 = _lib.launch_count('aux')
    dev = texture.vertex_normals(v.cuda(), f.cuda())
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') == n0 + 1
    assert dev.is_cuda and torch.equal(dev.cpu(), texture.vertex_normals(v, f))


def test_unused_vertices_and_a_degenerate_face(hip_lib):
    v, f, colors = two_sphere_scene()
    nv = len(v)
    v2 = torch.cat([v, torch.tensor([[0.0, 0.0, 0.0], [0.3, 0.3, 0.3]])])         # two vertices no proper face uses
    f2 = torch.cat([f, torch.tensor([[5, 5, 9], [nv, 7, nv]])])                  # a corner twice; an otherwise unused vertex twice
    c2 = torch.cat([colors, torch.tensor([[1, 2, 3], [4, 5, 6]], dtype=torch.uint8)])
    n_cpu = texture.vertex_normals(v2, f2)
    assert torch.equal(texture.vertex_normals(v2.cuda(), f2.cuda()).cpu(), n_cpu)
    assert torch.equal(n_cpu[nv:], torch.zeros([2, 3]))
    poses, cam = camera_kinds(2.2)['pinhole']
    proj = mesh.project(v2, poses, cam, 96)
    fid, dep = mesh.rasterize(proj, f2, 96)
    frames = mesh.shade(fid, proj, v2, f2, poses, c2, ambient=1.0)
    fallback = torch.randint(0, 256, [nv + 2, 3], generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    for min_cos in (0.1, 0.0):                                                   # (at 0 a zero normal may count, with weight 0: still the fallback)
        out, seen, _ = _parity((proj, fid, dep, frames, v2, n_cpu, poses), fallback=fallback, min_cos=min_cos)
        assert torch.equal(out[nv:], fallback[nv:])


def test_bake_matches_cpu_on_a_33_by_47_frame_and_one_vertex(hip_lib):
    for ortho in (False, True):
        inputs = soup_inputs(3, 33, 47, ortho=ortho)
        fallback = torch.randint(0, 256, [inputs[4].shape[0], 3], generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
        _, seen, _ = _parity(inputs, tolerance=0.4, fallback=fallback)
        assert (seen > 0).sum() > 20 and (seen == 0).sum() > 20
        _parity(inputs, tolerance=0.4, fallback=(7, 8, 9), groups=[(0, 1), (1, 3)])
        proj, fid, dep, frames, v, n, poses = inputs
        for i in (int(seen.argmax()), int(seen.argmin())):                        # V = 1: a vertex some view sees, and one none sees
            one = (mesh.Projection(proj.packed[:, i:i + 1].contiguous(), ortho), fid, dep, frames, v[i:i + 1], n[i:i + 1], poses)
            _, s1, _ = _parity(one, tolerance=0.4, fallback=(7, 8, 9))
            assert int(s1[0]) == int(seen[i])


@pytest.mark.parametrize('power,min_cos', [(1, 0.0), (4, 0.5), (8, 0.1)])
@pytest.mark.parametrize('per_vertex', [True, False])
def test_bake_matches_cpu_for_powers_thresholds_and_fallbacks(hip_lib, power, min_cos, per_vertex):
    inputs = _scene_buffers('two', 'pinhole')
    nv = inputs[4].shape[0]
    fallback = torch.randint(0, 256, [nv, 3], generator=torch.Generator().manual_seed(2), dtype=torch.uint8) if per_vertex else (11, 250, 0)
    colors, seen, _ = _parity(inputs, power=power, min_cos=min_cos, fallback=fallback)
    unseen = seen == 0
    assert unseen.any() and torch.equal(colors[unseen], fallback[unseen] if per_vertex else torch.tensor([[11, 250, 0]], dtype=torch.uint8).expand(int(unseen.sum()), 3))


# ---- 9. chaining ----------------------------------------------------------------------------------------------------------------
def test_view_groups_chain_into_the_same_bytes_on_the_device(hip_lib):
    proj, fid, dep, frames, v, n, poses = _scene_buffers('sphere', 'pinhole')
    dev = (proj.to('cuda'), fid.cuda(), dep.cuda(), frames.cuda(), v.cuda(), n.cuda(), poses)
    runs = [run_bake('cuda', *dev, 0.01, 2, 0.1, (200, 200, 200), groups=[(s, min(s + g, 14)) for s in range(0, 14, g)]) for g in (1, 3, 14)]
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1]) and torch.equal(r[2], runs[0][2])
    vs, f, colors = sphere_scene()
    cam = camera_kinds(4.2647)['pinhole'][1]
    whole = texture.bake_colors(vs.cuda(), f.cuda(), frames.cuda(), poses, cam, return_seen=True)
    for max_bytes in (1, 3 * 16 * len(vs)):
        part = texture.bake_colors(vs.cuda(), f.cuda(), frames.cuda(), poses, cam, return_seen=True, max_bytes=max_bytes)
        assert torch.equal(part[0], whole[0]) and torch.equal(part[1], whole[1])
    assert (whole[1] > 0).all() and (whole[0].int() - colors.cuda().int()).abs().max() <= 2


# ---- 10. the whole pipeline -------------------------------------------------------------------------------------------------------
def test_textured_mesh_equals_a_cpu_bake_of_its_frames(hip_lib, tmp_path, monkeypatch):
    G, ws, thr = _median_mesh('seg2cat', 32)
    used = {}
    real = views.render_views

    def spy(G_, ws_, cams, **kw):
        used['cams'] = cams
        used['frames'] = real(G_, ws_, cams, **kw)
        return used['frames']
    monkeypatch.setattr(views, 'render_views', spy)
    path = tmp_path / 'cat.ply'
    n0 = _lib.launch_count('aux')
    v, f, colors, seen, frames = texture.textured_mesh(G, ws, 'seg2cat', resolution=32, threshold=thr, n_frames=4, image_size=128, n_views=3,
                                                       path=str(path))
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') > n0
    assert colors.is_cuda and colors.dtype == torch.uint8 and tuple(colors.shape) == (len(v), 3) and tuple(seen.shape) == (len(v),)
    assert tuple(frames.shape) == (4, 128, 128, 3) and frames.dtype == torch.uint8
    cams = used['cams'].cpu()
    assert tuple(cams.shape) == (3, 25) and tuple(used['frames']['image'].shape) == (3, G.img_resolution, G.img_resolution, 3)
    rgb = texture.vertex_rgb(G, ws, v)
    ref, ref_seen = texture.bake_colors(v.cpu(), f.cpu(), used['frames']['image'].cpu(), cams[:, :16].reshape(-1, 4, 4), mesh.Pinhole(cams[:, 16:25]),
                                        fallback=rgb.cpu(), return_seen=True)
    assert torch.equal(seen.cpu(), ref_seen) and torch.equal(colors.cpu(), ref)
    assert (seen > 0).any() and (seen == 0).any() and torch.equal(colors[seen == 0], rgb[seen == 0])
    poses, camera = mesh.script_turntable(G, 4)
    grey = mesh.render(v, f, poses, camera, 128)
    assert not torch.equal(frames, grey) and ((grey != 255).any(-1).sum(dim=(1, 2)) > 100).all()
    data = open(path, 'rb').read()
    header = data[:data.index(b'end_header\n')].decode('ascii')
    assert f'element vertex {len(v)}' in header and 'property float nx' in header and 'property uchar red' in header
    assert len(data) == len(header) + len('end_header\n') + len(v) * 27 + len(f) * 13


def test_textured_mesh_colours_an_edge_generator(hip_lib):
    G, ws, thr = _median_mesh('edge2car', 32)
    assert mesh.extract_mesh(G, ws, resolution=32, threshold=thr, n_frames=2, image_size=64)[2] is None
    v, f, colors, seen, frames = texture.textured_mesh(G, ws, 'edge2car', resolution=32, threshold=thr, n_frames=2, image_size=64, n_views=3)
    assert colors is not None and colors.dtype == torch.uint8 and tuple(colors.shape) == (len(v), 3) and len(v) > 100
    assert len(colors.unique(dim=0)) > 1 and tuple(frames.shape) == (2, 64, 64, 3)


# ---- 11. a larger run -------------------------------------------------------------------------------------------------------------
def test_large_mesh_repeats_and_does_not_depend_on_the_face_order(hip_lib):
    """A 256-lattice gyroid ball, 8 views at 512^2: two runs give the same bytes, and so does a run with the faces shuffled."""
    v, f = _mc_mesh(_gyroid_ball(256, 100.0, 2.5))
    assert len(f) > 2_000_000
    v, f = v.cuda(), f.cuda()
    colors = true_colors(v.cpu()).cuda()
    poses = mesh.turntable_poses([0, 0, 0], 1.0, 8, yaw_range=1.5, pitch_range=0.8)
    cam = mesh.Orthographic(0.5, 0.5)
    frames = mesh.render(v, f, poses, cam, 512, colors=colors, ambient=1.0)
    a, sa = texture.bake_colors(v, f, frames, poses, cam, return_seen=True)
    b, sb = texture.bake_colors(v, f, frames, poses, cam, return_seen=True)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    print(f'{len(v)} vertices, {int((sa > 0).sum())} seen')
    assert int((sa > 0).sum()) > 10_000
    perm = torch.randperm(len(f), generator=torch.Generator().manual_seed(0)).cuda()
    c, sc = texture.bake_colors(v, f[perm], frames, poses, cam, return_seen=True)
    # the corner lists change with the face ids, so the fp64 sums of the normals are taken in another order; measured on an MI355X, the
    # fp32 normals, the colours and seen all come out identical here (1,373,144 vertices, 283,345 of them seen), so exact equality is
    # asserted rather than the 1 level the order of an fp64 sum could cost
    assert torch.equal(texture.vertex_normals(v, f), texture.vertex_normals(v, f[perm]))
    assert torch.equal(sa, sc)
    assert torch.equal(a, c)
