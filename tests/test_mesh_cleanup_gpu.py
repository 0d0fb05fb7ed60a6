"""pix2pix3d_amd.mesh clean-up on the device: p3d_mesh_components and the three clustering kernels against the CPU path (labels and
faces exactly, cluster means to one fp32 ulp), the launch bound of the union-find, determinism, and extract_mesh with clean-up on the
seeded generators."""
import math

import numpy as np
import pytest
import torch

from conftest import record_error
from pix2pix3d_amd import _lib, mesh, shape
from test_mesh_cleanup_host import fan, plate, spheres_field, strips, three_spheres
from test_mesh_gpu import _gyroid_ball, _median_mesh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cat128(hip_lib):
    """The seeded seg2cat generator's mesh at the median of its 128^3 field, world coordinates, with its CPU copy and the CPU labels.
    Thousands of components.  Shared: do not modify."""
    G, ws, thr = _median_mesh('seg2cat', 128)
    v, f = shape.extract_geometry(G, ws, 128, thr)
    vc, fc = v.cpu(), f.cpu()
    step = G.rendering_kwargs['box_warp'] / 127.0                              # one lattice step in world units
    return dict(v=v, f=f, vc=vc, fc=fc, labels=mesh.components(fc, len(vc)), step=step)


def _components_case(name):
    if name == 'spheres':
        v, f = three_spheres()
        return f, len(v), None
    if name == 'strip':
        return strips(1, 100_000)
    if name == 'strips':
        return strips(1000, 100)
    if name == 'fan':
        f, nv = fan(50_000)
        return f, nv, torch.zeros([nv], dtype=torch.int64)
    v, f = shape.marching_cubes(_gyroid_ball(96, 38.0, 2.5), 0.0)
    return f, len(v), None


@pytest.mark.parametrize('name', ['spheres', 'strip', 'strips', 'fan', 'gyroid'])
def test_components_match_cpu(hip_lib, name):
    faces, nv, expected = _components_case(name)
    cpu = mesh.components(faces, nv)
    if expected is not None:
        assert torch.equal(cpu, expected)
    n0 = _lib.launch_count('aux')
    dev = mesh.components(faces.cuda(), nv)
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') > n0
    assert dev.is_cuda and dev.dtype == torch.int64 and torch.equal(dev.cpu(), cpu)
    if name == 'gyroid':
        assert len(faces) > 256 * 64                                            # many work-groups


def test_components_seg2cat_mesh_128(hip_lib, cat128):
    assert len(cat128['labels'].unique()) > 1000 and len(cat128['fc']) > 100_000
    dev = mesh.components(cat128['f'], len(cat128['v']))
    assert torch.equal(dev.cpu(), cat128['labels'])
    back = torch.arange(len(cat128['fc']) - 1, -1, -1, device='cuda')
    assert torch.equal(mesh.components(cat128['f'][back], len(cat128['v'])), dev)                    # face order does not matter


def test_components_launch_bound(hip_lib):
    faces, nv, expected = strips(1, 100_000)
    faces = faces.cuda()
    torch.cuda.synchronize()
    n0 = _lib.launch_count('aux')
    dev = mesh.components(faces, nv)
    torch.cuda.synchronize()
    launches = _lib.launch_count('aux') - n0
    bound = 16 * math.ceil(math.log2(nv)) + 16
    assert bound == 288
    assert 1 <= launches <= bound, launches                                     # O(log V) rounds at most: label propagation needs ~12 675
    assert torch.equal(dev.cpu(), expected)


def test_cleanup_is_deterministic(hip_lib, cat128):
    v, f, step = cat128['v'], cat128['f'], cat128['step']
    same = lambda a, b: all(torch.equal(x.view(torch.int32) if x.is_floating_point() else x, y.view(torch.int32) if y.is_floating_point() else y)   # noqa: E731
                            for x, y in zip(a, b))
    assert torch.equal(mesh.components(f, len(v)), mesh.components(f, len(v)))
    assert same(mesh.clean(v, f, keep=3), mesh.clean(v, f, keep=3))
    assert same(mesh.simplify(v, f, 2 * step), mesh.simplify(v, f, 2 * step))


@pytest.mark.parametrize('keep,min_faces', [(1, 1), (None, 100)])
def test_clean_matches_cpu(hip_lib, cat128, keep, min_faces):
    cpu = mesh.clean(cat128['vc'], cat128['fc'], keep=keep, min_faces=min_faces)
    dev = mesh.clean(cat128['v'], cat128['f'], keep=keep, min_faces=min_faces)
    assert all(d.is_cuda for d in dev)
    assert torch.equal(dev[0].cpu().view(torch.int32), cpu[0].view(torch.int32))
    assert torch.equal(dev[1].cpu(), cpu[1]) and torch.equal(dev[2].cpu(), cpu[2])
    assert 0 < len(cpu[1]) < len(cat128['fc'])
    left = mesh.components(dev[1], len(dev[0])).unique()
    assert len(left) == 1 if keep == 1 else len(left) > 1


def test_clean_three_spheres_on_the_device(hip_lib):
    v, f = three_spheres()
    for keep, which in ((1, (0,)), (2, (0, 1))):
        want_v, want_f = shape.marching_cubes(spheres_field(which), 0.0)
        cv, cf, kept = mesh.clean(v.cuda(), f.cuda(), keep=keep)
        assert torch.equal(cv.cpu().view(torch.int32), want_v.view(torch.int32)) and torch.equal(cf.cpu(), want_f)
        assert torch.equal(v[kept.cpu()], want_v)


def _simplify_case(name, cat128):
    if name == 'spheres':
        return three_spheres() + ((2.0, 4.0),)
    if name == 'plate':
        return plate() + ((2.0, 1.0),)
    return cat128['vc'], cat128['fc'], (2 * cat128['step'], 4 * cat128['step'])


@pytest.mark.parametrize('name', ['spheres', 'plate', 'seg2cat128'])
def test_simplify_matches_cpu(hip_lib, cat128, name):
    v, f, cells = _simplify_case(name, cat128)
    vd, fd = v.cuda(), f.cuda()
    ulp = float(np.spacing(np.float32(v.abs().max())))                          # one fp32 ulp of the largest coordinate magnitude
    worst = 0.0
    for cell in cells:
        cv, cf = mesh.simplify(v, f, cell)
        n0 = _lib.launch_count('aux')
        dv, df = mesh.simplify(vd, fd, cell)
        torch.cuda.synchronize()
        assert _lib.launch_count('aux') >= n0 + 3
        assert dv.is_cuda and df.is_cuda and df.dtype == torch.int64 and dv.dtype == torch.float32
        assert torch.equal(df.cpu(), cf)
        assert dv.shape == cv.shape
        err = float((dv.cpu().double() - cv.double()).abs().max())
        worst = max(worst, err / ulp)
        assert 0 < len(cf) < len(f)
    record_error(f'mesh.simplify.{name}.vertices_ulp', worst)
    assert worst <= 1.0, worst                                                  # (both sum in ascending vertex id: 0 is expected)


@pytest.mark.parametrize('name', ['seg2cat', 'edge2car'])
def test_extract_mesh_with_cleanup(hip_lib, name):
    G, ws, thr = _median_mesh(name, 128)
    step = G.rendering_kwargs['box_warp'] / 127.0
    _, f0, _, _ = mesh.extract_mesh(G, ws, resolution=128, threshold=thr, n_frames=4)
    n0 = _lib.launch_count('aux')
    v, f, colors, frames = mesh.extract_mesh(G, ws, resolution=128, threshold=thr, n_frames=4, keep=1, cell=2 * step)
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') > n0
    assert 0 < len(f) < len(f0)
    assert f.dtype == torch.int64 and int(f.min()) >= 0 and int(f.max()) < len(v)
    assert len(mesh.components(f, len(v)).unique()) == 1                                          # one component, no stray vertex
    if name == 'seg2cat':
        assert colors.shape == (len(v), 3) and colors.dtype == torch.uint8
        assert torch.equal(colors, mesh.vertex_labels(G, ws, v)[1])                                  # labelled AFTER the clean-up
    else:
        assert colors is None
    assert frames.shape == (4, 512, 512, 3) and frames.is_cuda and frames.dtype == torch.uint8
    background = (frames == 255).all(-1)
    assert bool(((~background).sum(dim=(1, 2)) > 0).all())
