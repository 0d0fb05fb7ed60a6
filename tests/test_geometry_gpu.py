"""pix2pix3d_amd.geometry on the device against the CPU definition: d2 bits and face ids of the tree walk on one triangle and the
degenerate faces, at the tree's size boundaries, on spread-out clusters with ties and bad faces, and across many work-groups; the
samples' bytes; compare and simplify_to; the pipelines' tolerance=."""
import pytest
import torch

import geometry_cases as cases
from pix2pix3d_amd import _lib, geometry, mesh
from test_mesh_gpu import _gyroid_ball
from test_shape_host import sphere

pytestmark = pytest.mark.gpu
LEAF = geometry.LEAF


def _same(got, want):
    assert got.d2.is_cuda and got.d2.dtype == torch.float64 and got.face.dtype == torch.int64
    assert torch.equal(got.d2.cpu().view(torch.int64), want.d2.view(torch.int64))
    assert torch.equal(got.face.cpu(), want.face)


def _both(points, v, f, **kw):
    n0 = _lib.launch_count('aux')
    got = geometry.closest(points.cuda(), v.cuda(), f.cuda(), **kw)
    torch.cuda.synchronize()
    assert _lib.launch_count('aux') > n0                                   # the kernels ran
    want = geometry.closest(points, v, f)
    _same(got, want)
    return want


def test_pair_paths_on_one_triangle_and_the_degenerate_faces():
    pts = cases.region_points(4096, 1)
    v = torch.tensor(cases.REGION_TRIANGLE, dtype=torch.float32)
    want = _both(pts, v, torch.tensor([[0, 1, 2]]))
    assert bool((want.face == 0).all()) and int((want.d2 == 0).sum()) >= 6
    for face in cases.DEGENERATE_FACES:
        _both(pts * 4 - 2, torch.tensor(face, dtype=torch.float32), torch.tensor([[0, 1, 2]]))
    allv = torch.tensor([c for face in cases.DEGENERATE_FACES for c in face], dtype=torch.float32)
    _both(pts * 4 - 2, allv, torch.arange(12).reshape(4, 3))


@pytest.mark.parametrize('n_faces', [1, LEAF, LEAF + 1, 2 * LEAF + 1, 63, 64, 65, 257])
def test_tree_boundaries(n_faces):
    v, f = cases.soup(n_faces, 100 + n_faces)
    for n in (1, 63, 64, 65, 1000):
        pts = cases.cloud(n, n)
        want = _both(pts, v, f, sort_queries=bool(n % 2))
        assert bool((want.face >= 0).all())


def test_spread_ties_and_bad_faces():
    pts, v, f = cases.spread_case()
    want = _both(pts, v, f)
    assert bool((want.face[-2:] == -1).all()) and bool((want.face[:-2] >= 0).all()) and bool((want.face < 70).all())
    _both(pts, v, f, sort_queries=True)
    none = geometry.closest(pts.cuda(), v.cuda(), f[-3:].cuda())           # no valid face
    assert bool(torch.isinf(none.d2).all()) and bool((none.face == -1).all())
    empty = geometry.closest(pts.cuda(), v.cuda(), f[:0].cuda())
    assert bool(torch.isinf(empty.d2).all()) and bool((empty.face == -1).all())
    assert geometry.closest(pts[:0].cuda(), v.cuda(), f.cuda()).d2.shape == (0,)


def test_many_work_groups_and_order_independence():
    (va, fa), (vb, fb) = cases.sphere_mesh(14.2), cases.sphere_mesh(17.7)
    s = geometry.surface_samples(va.cuda(), fa.cuda(), 0.45)
    assert len(s.points) >= 65536
    bvh = geometry.build_bvh(vb.cuda(), fb.cuda())
    got = geometry.closest(s.points, None, None, bvh=bvh)
    pick = torch.arange(0, len(s.points), len(s.points) // 2000)
    want = geometry.closest(s.points[pick].cpu(), vb, fb)
    assert torch.equal(got.d2[pick].cpu().view(torch.int64), want.d2.view(torch.int64)) and torch.equal(got.face[pick].cpu(), want.face)
    assert float((got.d2.sqrt() - 3.5).abs().max()) < 0.1
    unsorted = geometry.closest(s.points, None, None, bvh=bvh, sort_queries=False)
    assert torch.equal(unsorted.d2, got.d2) and torch.equal(unsorted.face, got.face)
    back = geometry.closest(s.points.flip(0), vb.cuda(), fb.cuda().flip(0))
    assert torch.equal(back.d2.flip(0), got.d2)
    mapped = (len(fb) - 1 - back.face.flip(0))[pick].cpu()                 # the ids map back: the same face, or (a closest point on a
    corners = vb.double()[fb[mapped]]                                      # shared edge) another at exactly the same distance
    p = tuple(x for x in s.points[pick].cpu().double().unbind(1))
    again = geometry.tri_d2(p, *[tuple(corners[:, j].unbind(1)) for j in range(3)])
    assert torch.equal(again.view(torch.int64), want.d2.view(torch.int64)) and float((mapped == want.face).float().mean()) > 0.5


def test_samples_equal_the_cpu_formulation():
    u = _gyroid_ball(40, 17.0, 3.0)
    v, f = mesh.shape.marching_cubes(u, 0.0)
    v = v / 39 - 0.5
    for spacing, k_max in ((0.02, 64), (0.004, 3)):
        n0 = _lib.launch_count('aux')
        got = geometry.surface_samples(v.cuda(), f.cuda(), spacing, k_max)
        assert _lib.launch_count('aux') == n0 + 2
        want = geometry.surface_samples(v, f, spacing, k_max)
        assert torch.equal(got.points.cpu().view(torch.int32), want.points.view(torch.int32)) and torch.equal(got.face.cpu(), want.face)
        assert int(got.capped) == int(want.capped)
    assert int(want.capped) > 0
    for k in (1, 2, 3, 7, 64):                                             # the predicate's boundaries
        t = torch.tensor([[0, 0, 0], [3 * k, 0, 0], [0, 4 * k, 0]], dtype=torch.float32)
        for spacing in (5.0, 4.999999999999999):
            got, want = (geometry.surface_samples(t.to(d), torch.tensor([[0, 1, 2], [2, 1, 7], [0, 2, 1]]).to(d), spacing) for d in ('cuda', 'cpu'))
            assert torch.equal(got.points.cpu().view(torch.int32), want.points.view(torch.int32)) and torch.equal(got.face.cpu(), want.face)
            assert int(got.capped) == int(want.capped) and len(got.points) == 2 * min(k + (spacing < 5), 64) ** 2


def test_compare_and_simplify_to_equal_the_cpu():
    (va, fa), (vb, fb) = cases.small_sphere(6.1), cases.small_sphere(9.6)
    thresholds = (3.45, 3.5, 3.55)
    got, want = geometry.compare(va.cuda(), fa.cuda(), vb.cuda(), fb.cuda(), 1.5, thresholds), geometry.compare(va, fa, vb, fb, 1.5, thresholds)
    for g, w in ((got.forward, want.forward), (got.backward, want.backward)):
        assert g.within.is_cuda and g.within.dtype == torch.int64 and g.within.tolist() == w.within.tolist() and g.n == w.n
        assert float(g.max) == float(w.max)
        assert abs(float(g.mean) - float(w.mean)) <= 1e-12 * float(w.mean) and abs(float(g.rms) - float(w.rms)) <= 1e-12 * float(w.rms)
    assert float(got.hausdorff) == float(want.hausdorff) and abs(float(got.chamfer) - float(want.chamfer)) <= 1e-12 * float(want.chamfer)
    assert torch.equal(got.fscore.cpu(), want.fscore)
    dv, df, dcell, dagree = mesh.simplify_to(va.cuda(), fa.cuda(), 0.5, 1.5)
    cv, cf, ccell, cagree = mesh.simplify_to(va, fa, 0.5, 1.5)
    assert dcell == ccell and torch.equal(dv.cpu(), cv) and torch.equal(df.cpu(), cf)
    assert float(dagree.hausdorff) == float(cagree.hausdorff) and dagree.forward.within.tolist() == cagree.forward.within.tolist()
    col = geometry.distance_colors(geometry.closest(vb.cuda(), va.cuda(), fa.cuda()).d2, 4.0)
    assert torch.equal(col.cpu(), geometry.distance_colors(geometry.closest(vb, va, fa).d2, 4.0))


def test_pipelines_take_a_tolerance_and_change_map():
    from test_texture_host import small_generator
    G, ws, thr = small_generator('seg2cat', device='cuda')
    kw = dict(resolution=32, threshold=thr, n_frames=2, image_size=64)
    v0, f0 = mesh._clean_geometry(G, ws, 32, thr, None, 1, None)
    tolerance = 0.02 * geometry.diagonal(v0)
    v, f, colors, frames = mesh.extract_mesh(G, ws, tolerance=tolerance, **kw)
    assert 0 < len(f) <= len(f0) and frames.shape == (2, 64, 64, 3) and len(colors) == len(v)      # (a noisy seeded mesh: no rung need cut faces)
    assert float(geometry.compare(v0, f0, v, f, thresholds=(tolerance,)).hausdorff) <= tolerance
    change = geometry.change_map(G, ws, ws * 1.05, resolution=32, threshold=thr, n_frames=2, image_size=64)
    assert change.d2.shape == (len(change.vertices),) and change.colors.shape == (len(change.vertices), 3) and change.frames.shape == (2, 64, 64, 3)
    assert float(change.agreement.hausdorff) > 0 and not (change.frames == 255).all()
    same = geometry.change_map(G, ws, ws, resolution=32, threshold=thr)
    assert same.frames is None and float(same.agreement.hausdorff) < 1e-6 and bool((same.colors == 0).all())
