"""csrc/mesh_atlas.hip against the CPU formulation of pix2pix3d_amd/atlas.py: texel geometry, the assembled image and the albedo bit for
bit, a shaded frame within the headlight term's one level; the bake chained from the existing kernels; a larger run; atlas_mesh."""
import numpy as np
import pytest
import torch

from pix2pix3d_amd import _lib, atlas, mesh, texture
from test_atlas_host import baked, oriented, scene_views, shade_case
from test_mesh_host import grouped_views
from test_mesh_gpu import _gyroid_ball, _mc_mesh, _median_mesh
from test_texture_host import camera_kinds, true_colors

pytestmark = pytest.mark.gpu


def _one_launch(fn):
    n0 = _lib.launch_count('aux')
    out = fn()
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') == n0 + 1
    return out


# ---- 1. texel geometry and assembly ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,n_faces,size', [('sphere', None, 336), ('sphere', None, 512), ('two', None, 256), ('two', 1, 16), ('two', 2, 16),
                                               ('two', 301, 110), ('two', 300, 64)])
def test_texel_points_and_assemble_match_cpu(hip_lib, name, n_faces, size):
    v, f, _, n = oriented(name)
    f = f[:n_faces].clone()
    if n_faces == 300:
        f[17, 2] = len(v)                                                      # an index out of range
    lay = atlas.layout(len(f), size)
    assert (lay.cell, lay.side) == {336: (4, 1), 512: (6, 3), 256: (5, 2), 16: (16, 13), 110: (8, 5), 64: (4, 1)}[size]
    assert size != 110 or lay.per_row * lay.cell < size                        # unused margins
    cpu = atlas.texel_points(v, f, n, lay)
    dev = _one_launch(lambda: atlas.texel_points(v.cuda(), f.cuda(), n.cuda(), lay))
    for a, b, what in zip(dev, cpu, ('points', 'normals', 'face')):
        assert a.is_cuda and a.dtype == b.dtype and torch.equal(a.cpu(), b), what
    assert (cpu[2] == -1).any() == (n_faces in (1, 301, 300))
    colors = torch.randint(0, 256, [lay.n_texels, 3], generator=torch.Generator().manual_seed(size), dtype=torch.uint8)
    want = atlas.assemble(colors, cpu[2], lay, background=(3, 200, 77))
    got = _one_launch(lambda: atlas.assemble(colors.cuda(), dev[2], lay, background=(3, 200, 77)))
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (size, size, 3) and torch.equal(got.cpu(), want)


# ---- 2. the bake ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
@pytest.mark.parametrize('name,size', [('sphere', 512), ('two', 256)])
def test_bake_texture_matches_cpu(hip_lib, name, size, kind):
    v, f, _, n = oriented(name)
    poses, cam, frames = scene_views(name, kind)
    lay, tex, seen = baked(name, kind, size)
    n0 = _lib.launch_count('aux')
    got, got_seen = atlas.bake_texture(v.cuda(), f.cuda(), frames.cuda(), poses, cam, lay, normals=n.cuda())
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') >= n0 + 5
    assert got.is_cuda and got_seen.is_cuda and got.dtype == torch.uint8 and got_seen.dtype == torch.int32
    assert torch.equal(got_seen.cpu(), seen), 'seen'
    assert torch.equal(got.cpu(), tex), 'texture'
    part, part_seen = atlas.bake_texture(v.cuda(), f.cuda(), frames.cuda(), poses, cam, size, normals=n.cuda(), max_bytes=1)
    assert torch.equal(part, got) and torch.equal(part_seen, got_seen)         # one view per group: the same bytes


# ---- 3. the textured shade ----------------------------------------------------------------------------------------------------------
def _shade_parity(fid, proj, v, f, poses, tex, lay):
    dev = (fid.cuda(), proj.to('cuda'), v.cuda(), f.cuda(), poses, tex.cuda(), lay)
    want = atlas.shade_textured(fid, proj, v, f, poses, tex, lay, background=(10, 255, 0), ambient=1.0)
    got = _one_launch(lambda: atlas.shade_textured(*dev, background=(10, 255, 0), ambient=1.0))
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), want)      # the albedo is an exact integer ratio, the factor exactly 1
    want = atlas.shade_textured(fid, proj, v, f, poses, tex, lay, background=(10, 255, 0), ambient=0.25)
    got = _one_launch(lambda: atlas.shade_textured(*dev, background=(10, 255, 0), ambient=0.25))
    diff = (got.cpu().int() - want.int()).abs()
    print(f'ambient 0.25: {int((diff > 0).sum())} of {diff.numel()} bytes differ, by at most {int(diff.max())}')
    assert int(diff.max()) <= 1                                                # the headlight term: test_shade_matches_cpu's bound


@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
def test_shade_textured_matches_cpu_on_a_33_by_47_frame(hip_lib, kind):
    _shade_parity(*shade_case(kind))


@pytest.mark.parametrize('kind', ['ortho', 'pinhole'])
def test_shade_textured_matches_cpu_on_300_by_300_frames(hip_lib, kind):
    v, f, _, _ = oriented('sphere')
    poses, cam = camera_kinds(4.2647)[kind]
    lay = atlas.layout(len(f), 512)
    tex = torch.randint(0, 256, [512, 512, 3], generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    proj = mesh.project(v, poses[:3], cam, 300)
    fid, _ = mesh.rasterize(proj, f, 300)
    assert (fid >= 0).sum() > 50_000
    _shade_parity(fid, proj, v, f, poses[:3], tex, lay)


# ---- 4. devices -------------------------------------------------------------------------------------------------------------------
def test_shade_textured_moves_inputs_to_the_face_id_device(hip_lib):
    fid, proj, v, f, poses, tex, lay = shade_case('ortho')
    mixed = atlas.shade_textured(fid.cuda(), proj, v, f, poses, tex, lay)
    same = atlas.shade_textured(fid.cuda(), proj.to('cuda'), v.cuda(), f.cuda(), poses, tex.cuda(), lay)
    assert mixed.is_cuda and torch.equal(mixed, same)
    back = atlas.shade_textured(fid, proj.to('cuda'), v.cuda(), f, poses, tex.cuda(), lay)
    assert not back.is_cuda and (back.int() - mixed.cpu().int()).abs().max() <= 1


# ---- 5. view groups: launches and slicing ---------------------------------------------------------------------------------------------
_group_cases = {}


def _group_case(call):
    """(run(device, max_bytes) -> tensors, points per view, launches of g groups) of one whole-pipeline call on test_mesh_host.py's
    three views with per-frame intrinsics; on the device the poses and the intrinsics are device tensors too."""
    if not _group_cases:
        v, f, colors, poses, cam = grouped_views()
        f = atlas.orient_faces(v, f)
        lay = atlas.layout(len(f), 256)
        tex = torch.randint(0, 256, [256, 256, 3], generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
        frames = mesh.render(v, f, poses, cam, 96, colors=colors, ambient=1.0)
        normals = texture.vertex_normals(v, f)

        def on(device):
            return [t.to(device) for t in (v, f, colors, poses, cam.intrinsics, tex, frames, normals)]

        def render(device, max_bytes):
            v, f, colors, poses, k, _, _, _ = on(device)
            return (mesh.render(v, f, poses, mesh.Pinhole(k), 96, colors=colors, ambient=1.0, max_bytes=max_bytes),)

        def render_textured(device, max_bytes):
            v, f, _, poses, k, tex, _, _ = on(device)
            return (atlas.render_textured(v, f, poses, mesh.Pinhole(k), 96, tex, lay, ambient=1.0, max_bytes=max_bytes),)

        def bake_colors(device, max_bytes):
            v, f, _, poses, k, _, frames, _ = on(device)
            return texture.bake_colors(v, f, frames, poses, mesh.Pinhole(k), return_seen=True, max_bytes=max_bytes)

        def bake_texture(device, max_bytes):
            v, f, _, poses, k, _, frames, normals = on(device)
            return atlas.bake_texture(v, f, frames, poses, mesh.Pinhole(k), lay, normals=normals, max_bytes=max_bytes)
        # project, count, bin, raster + shade per group; the bakes: accumulate per group (bake_texture: and the texels' projection), the
        # finish, and the normals (bake_colors) or the texels and the assembly (bake_texture)
        _group_cases.update(render=(render, len(v), lambda g: 5 * g), render_textured=(render_textured, len(v), lambda g: 5 * g),
                            bake_colors=(bake_colors, len(v), lambda g: 5 * g + 2),
                            bake_texture=(bake_texture, lay.n_texels, lambda g: 6 * g + 3))
    return _group_cases[call]


@pytest.mark.parametrize('call', ['render', 'render_textured', 'bake_colors', 'bake_texture'])
def test_view_groups_launch_counts_and_match_cpu(hip_lib, call):
    """One group of three views and three groups of one: the aux launches of each, and the bytes of the CPU path from the three groups
    (ambient = 1, so that the shade's factor is exactly 1 on both paths)."""
    run, n_points, launches = _group_case(call)
    for groups, max_bytes in ((1, 3 * 16 * n_points), (3, 1)):
        n0 = _lib.launch_count('aux')
        got = run('cuda', max_bytes)
        torch.cuda.synchronize()
        count = _lib.launch_count('aux') - n0
        assert count == launches(groups), (groups, count)
    want = run('cpu', 1 << 30)
    for a, b in zip(got, want):
        differ = int((a.cpu() != b).sum())
        assert a.is_cuda and a.dtype == b.dtype and differ == 0, f'{differ} of {b.numel()} elements differ from the CPU path'


# ---- 6. a larger run ----------------------------------------------------------------------------------------------------------------
def test_large_mesh_bakes_renders_and_repeats(hip_lib):
    """A 112-lattice gyroid ball (some 250 000 faces: cells of 5 texels at 2048^2), 8 views of 512^2, 8 turntable frames."""
    v, f = _mc_mesh(_gyroid_ball(112, 44.0, 2.5))
    assert 200_000 < len(f) < 280_000
    v, f = v.cuda(), f.cuda()
    f = atlas.orient_faces(v, f)
    colors = true_colors(v.cpu()).cuda()                                     # channels in 27 .. 228
    poses = mesh.turntable_poses([0, 0, 0], 1.0, 8, yaw_range=1.5, pitch_range=0.8)
    cam = mesh.Orthographic(0.5, 0.5)
    frames = mesh.render(v, f, poses, cam, 512, colors=colors, ambient=1.0)
    lay = atlas.layout(len(f), 2048)
    assert lay.cell == 5
    magenta = (255, 0, 255)
    runs = []
    for _ in range(2):
        tex, seen = atlas.bake_texture(v, f, frames, poses, cam, lay, fallback=(100, 100, 100), background=magenta)
        out, fid, _ = atlas.render_textured(v, f, poses, cam, 512, tex, lay, ambient=1.0, return_buffers=True)
        runs.append((tex, seen, out))
    torch.cuda.synchronize()
    tex, seen, out = runs[0]
    assert tex.is_cuda and tex.dtype == torch.uint8 and tuple(tex.shape) == (2048, 2048, 3)
    assert seen.is_cuda and seen.dtype == torch.int32 and tuple(seen.shape) == (lay.n_texels,)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (8, 512, 512, 3)
    print(f'{len(f)} faces, cell {lay.cell}, {int((seen > 0).sum())} of {lay.n_texels} texels seen')
    assert int((seen > 0).sum()) > 100_000
    on = fid >= 0
    assert (on.sum(dim=(1, 2)) > 50_000).all() and (out[~on] == 255).all()
    # no background colour on mesh pixels: a lookup mixes texels of its own face only, all of them baked colours (27 .. 228) or the
    # fallback, so no channel can reach the 255 or the 0 of the atlas's background
    assert int(out[on].min()) >= 27 and int(out[on].max()) <= 228
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)


# ---- 7. the whole pipeline ------------------------------------------------------------------------------------------------------------
def test_atlas_mesh_on_a_device_generator(hip_lib, tmp_path):
    from PIL import Image
    G, ws, thr = _median_mesh('seg2cat', 32)
    path = tmp_path / 'cat.obj'
    n0 = _lib.launch_count('aux')
    v, f, lay, tex, seen, frames = atlas.atlas_mesh(G, ws, 'seg2cat', size=512, resolution=32, threshold=thr, n_frames=4, image_size=128,
                                                    keep=1, cell=0.08, n_views=3, path=str(path))
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') > n0
    assert len(f) > 500 and lay == atlas.layout(len(f), 512) and torch.equal(atlas.orient_faces(v, f), f)
    assert all(t.is_cuda for t in (v, f, tex, seen, frames))
    assert tex.dtype == torch.uint8 and tuple(tex.shape) == (512, 512, 3) and tuple(seen.shape) == (lay.n_texels,)
    assert tuple(frames.shape) == (4, 128, 128, 3) and frames.dtype == torch.uint8 and (seen > 0).any()
    poses, camera = mesh.script_turntable(G, 4)
    ref, fid, _ = atlas.render_textured(v.cpu(), f.cpu(), poses, camera, 128, tex.cpu(), lay, return_buffers=True)
    assert ((fid >= 0).sum(dim=(1, 2)) > 100).all()
    assert (frames.cpu().int() - ref.int()).abs().max() <= 1
    assert sorted(p.name for p in tmp_path.iterdir()) == ['cat.mtl', 'cat.obj', 'cat.png']
    text = open(path).read()
    assert text.count('\nv ') == len(v) and text.count('\nvn ') == len(v) and text.count('\nvt ') == 3 * len(f) and text.count('\nf ') == len(f)
    assert 'map_Kd cat.png' in open(tmp_path / 'cat.mtl').read()
    assert torch.equal(torch.from_numpy(np.asarray(Image.open(tmp_path / 'cat.png').convert('RGB')).copy()), tex.cpu())
