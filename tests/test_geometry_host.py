"""pix2pix3d_amd.geometry on CPU tensors, the definition: tri_d2 against exact rational arithmetic, closest against a plain double loop,
surface_samples against a per-face loop and at the boundaries of its integer predicate, the metrics on two concentric spheres against
the analytic distance, simplify_to's post-condition, the colour table, and the argument checks of the five entry points."""
import ctypes
import itertools
import math
from fractions import Fraction

import pytest
import torch

import geometry_cases as cases
from pix2pix3d_amd import _lib, geometry, mesh
from test_mesh_cleanup_host import three_spheres


def _t(rows, dtype=torch.float32):
    return torch.tensor(rows, dtype=dtype)


def _as_xyz(rows):
    """float64 [N, 3] -> the tuple of three [N] tensors geometry.tri_d2 takes."""
    return tuple(torch.tensor(rows, dtype=torch.float64).unbind(1))


# ---- tri_d2 ---------------------------------------------------------------------------------------------------------------------
def _region(p, a, b, c):
    """Which of the seven Voronoi regions of the triangle the projection of p falls in: the signs of its barycentrics."""
    F = Fraction
    e1, e2, r = [F(y - x) for x, y in zip(a, b)], [F(y - x) for x, y in zip(a, c)], [F(y - x) for x, y in zip(a, p)]
    fdot = lambda u, v: sum(x * y for x, y in zip(u, v))                  # noqa: E731
    d11, d12, d22, r1, r2 = fdot(e1, e1), fdot(e1, e2), fdot(e2, e2), fdot(r, e1), fdot(r, e2)
    det = d11 * d22 - d12 * d12
    u, v = (d22 * r1 - d12 * r2) / det, (d11 * r2 - d12 * r1) / det
    return (u < 0, v < 0, u + v > 1)


def _tri_cases():
    flat = ((0, 0, 0), (12, 0, 0), (0, 12, 0))
    tilted = ((-64, 3, 10), (40, -22, 64), (7, 60, -31))
    out = []
    for x, y, z in itertools.product(range(-6, 19, 3), range(-6, 19, 3), (-5, 0, 7)):       # edges, vertices and the plane included
        out.append(((x, y, z),) + flat)
    for x, y, z in itertools.product(range(-64, 65, 16), repeat=3):
        out.append(((x, y, z),) + tilted)
    for face in cases.DEGENERATE_FACES:
        for x, y, z in itertools.product(range(-8, 9, 4), repeat=3):
            out.append(((x, y, z),) + face)
        out.extend((corner,) + face for corner in face)
    return out, (flat, tilted)


def test_tri_d2_against_exact_arithmetic():
    """Integer coordinates, |x| <= 64: points in all seven Voronoi regions of two triangles, on their edges, vertices and planes, and
    about a point face, a segment face, a collinear face and a sliver.  |tri_d2 - exact| <= c 2^-53 S^2 with S the largest coordinate
    difference of the case.  Measured here: the worst ratio over these cases is 3.413; c is set to 4 x that, 13.66.  (With
    integer inputs every product and sum up to the quotients is exact, so the error is that of one division, one multiply-subtract
    per component and the final dot product.)"""
    tri_cases, proper = _tri_cases()
    for tri in proper:
        assert len({_region(p, *tri) for p, *t in tri_cases if tuple(t) == tri}) == 7
    got = geometry.tri_d2(*[_as_xyz([c[k] for c in tri_cases]) for k in range(4)])
    assert got.dtype == torch.float64 and bool(torch.isfinite(got).all())
    worst = 0.0
    for (p, a, b, c), d in zip(tri_cases, got.tolist()):
        assert d == cases.tri_d2(*[tuple(float(x) for x in q) for q in (p, a, b, c)])      # the Python restatement: the same bits
        exact = cases.exact_d2(p, a, b, c)
        span = max(abs(x - y) for q in (p, a, b, c) for r in (p, a, b, c) for x, y in zip(q, r))
        ratio = float(abs(Fraction(d) - exact) / (Fraction(1, 2 ** 53) * span * span)) if span else float(d != 0)
        worst = max(worst, ratio)
        assert ratio <= 13.66, (p, a, b, c, d, float(exact), ratio)
    print(f'tri_d2: worst ratio {worst:.4f} over {len(tri_cases)} cases')
    on = [((6, 6, 0), 0), ((0, 0, 0), 0), ((4, 4, 0), 0), ((4, 4, 3), 9), ((-3, -4, 0), 25), ((15, 0, 0), 9)]       # edge, vertex, inside, above, off a vertex, off an end
    flat = proper[0]
    for p, want in on:
        assert cases.tri_d2(tuple(map(float, p)), *[tuple(map(float, q)) for q in flat]) == want


def _small_scene():
    v, f = cases.soup(12, 3, extent=6.0, size=2.5)
    v = torch.cat([v, _t([[float('nan'), 1.0, 2.0], [0.5, float('inf'), 0.0]])])
    f = torch.cat([f, f[2:5], torch.tensor([[0, 1, len(v) - 2], [3, len(v) - 1, 4], [0, 1, len(v)], [-1, 0, 2], [5, 5, 5], [6, 7, 6]])])
    pts = torch.cat([cases.cloud(25, 4, 9.0), v[f[:6]].mean(1), v[:4], _t([[float('nan'), 0, 0], [0, 0, float('-inf')]])])
    return pts, v, f


def test_closest_equals_the_double_loop():
    pts, v, f = _small_scene()
    got = geometry.closest(pts, v, f)
    d2, face = cases.closest_loop(pts, v, f)
    assert got.d2.dtype == torch.float64 and got.face.dtype == torch.int64
    assert torch.equal(got.d2.view(torch.int64), d2.view(torch.int64)) and torch.equal(got.face, face)
    assert bool((got.face[-2:] == -1).all()) and bool(torch.isinf(got.d2[-2:]).all())      # the non-finite points
    assert bool((got.face[:-2] >= 0).all()) and not bool(torch.isnan(got.d2).any())
    dup = (got.face >= 2) & (got.face <= 4)                                # faces 12..14 repeat 2..4: the smaller id wins
    assert bool(dup.any()) and not bool(((got.face >= 12) & (got.face <= 14)).any())
    assert not bool((got.face >= 15).any())                                # NaN corner, inf corner, index past V, negative index: never chosen ...
    assert bool((geometry.closest(v[[5, 6]], v, f).d2 == 0).all())         # ... while the point face and the segment face count
    # int32 faces, chunked pairs: the same
    again = geometry._closest_cpu(pts, v, f.to(torch.int32), pairs=64, face_chunk=5)
    assert torch.equal(again.d2, got.d2) and torch.equal(again.face, got.face)


def test_closest_without_faces_or_points():
    pts, v, f = _small_scene()
    none = geometry.closest(pts, v, f[:0])
    assert bool(torch.isinf(none.d2).all()) and bool((none.face == -1).all()) and none.d2.shape == (len(pts),)
    bad = geometry.closest(pts, v, torch.tensor([[0, 1, len(v)], [0, 1, len(v) - 2]]))      # no valid face at all
    assert bool(torch.isinf(bad.d2).all()) and bool((bad.face == -1).all())
    empty = geometry.closest(pts[:0], v, f)
    assert empty.d2.shape == (0,) and empty.face.shape == (0,) and empty.d2.dtype == torch.float64
    far = geometry.closest(pts[:3], v, torch.tensor([[0, 1, 2 ** 32 + 1]]))                # an int64 index must not wrap into range
    assert bool(torch.isinf(far.d2).all())
    with pytest.raises(ValueError):
        geometry.closest(pts[:, :2], v, f)
    with pytest.raises(ValueError):
        geometry.build_bvh(v, f)                                           # the hierarchy is the device's


# ---- surface samples ----------------------------------------------------------------------------------------------------------------
def _inside(points, face, v, f):
    """Every sample lies in its face's plane and inside it, to fp32 rounding."""
    a, b, c = (v[f[face][:, k]].double() for k in range(3))
    p = points.double()
    n = torch.linalg.cross(b - a, c - a)
    area2 = n.norm(dim=1)
    bary = [torch.linalg.cross(y - x, p - x).mul(n).sum(1) / area2 ** 2 for x, y in ((b, c), (c, a), (a, b))]
    scale = torch.stack([a, b, c]).abs().amax((0, 2))
    off_plane = ((p - a) * n).sum(1).abs() / area2
    return bool((torch.stack(bary) > 0).all()) and bool((off_plane <= 4e-7 * scale).all()) and bool(((sum(bary) - 1).abs() < 1e-5).all())


def test_surface_samples_at_the_predicates_boundaries():
    """Integer right triangles whose longest edge is exactly k spacing: k itself must do, and a spacing one ulp shorter needs k + 1."""
    spacing = 5.0
    for k in (1, 2, 3, 7, 64):
        v = _t([[0, 0, 0], [3 * k, 0, 0], [0, 4 * k, 0]])                 # edges 3 k, 4 k, 5 k
        f = torch.tensor([[0, 1, 2]])
        s = geometry.surface_samples(v, f, spacing)
        assert s.points.shape == (k * k, 3) and s.points.dtype == torch.float32 and s.face.dtype == torch.int64 and int(s.capped) == 0
        below = geometry.surface_samples(v, f, math.nextafter(spacing, 0.0))
        assert below.points.shape == (min(k + 1, 64) ** 2, 3) and int(below.capped) == (k == 64)
        assert _inside(s.points, s.face, v, f)
    # the cap and its count: the second face wants k = 10
    v = _t([[0, 0, 0], [3, 0, 0], [0, 4, 0], [30, 0, 0], [0, 40, 0]])
    f = torch.tensor([[0, 1, 2], [0, 3, 4], [0, 2, 1]])
    s = geometry.surface_samples(v, f, 5.0, k_max=4)
    assert torch.equal(torch.bincount(s.face), torch.tensor([1, 16, 1])) and int(s.capped) == 1 and s.capped.dtype == torch.int64
    assert int(geometry.surface_samples(v, f, 5.0, k_max=10).capped) == 0
    for bad in (dict(spacing=0.0), dict(spacing=float('nan')), dict(spacing=1e-200), dict(spacing=1.0, k_max=0), dict(spacing=1.0, k_max=geometry.K_MAX_CAP + 1)):
        with pytest.raises(ValueError):
            geometry.surface_samples(v, f, **bad)


def test_surface_samples_order_and_the_per_face_loop():
    v = _t([[0, 0, 0], [9, 0, 0], [0, 9, 0]])
    s = geometry.surface_samples(v, torch.tensor([[0, 1, 2]]), 3.0)       # the hypotenuse is 12.73: k = 5
    k = math.isqrt(len(s.points))
    want = [(3 * i + 1, 3 * j + 1) for i in range(k) for j in range(k - i)] + [(3 * i + 2, 3 * j + 2) for i in range(k - 1) for j in range(k - 1 - i)]
    # the point is (n0 a + n1 b + n2 c) / (3 k): with a = 0, b = 9 e_x, c = 9 e_y it reads off (n1, n2)
    got = [(3 * k - round(x * 3 * k / 9) - round(y * 3 * k / 9), round(x * 3 * k / 9)) for x, y, _ in s.points.tolist()]
    assert k == 5 and got == want
    pts, vv, ff = _small_scene()
    for spacing, k_max in ((0.9, 64), (0.2, 3)):
        got = geometry.surface_samples(vv, ff, spacing, k_max)
        points, face, capped = cases.samples_loop(vv, ff, spacing, k_max)
        assert torch.equal(got.points.view(torch.int32), points.view(torch.int32)) and torch.equal(got.face, face) and int(got.capped) == capped
    assert capped > 0 and not bool(((got.face >= 15) & (got.face <= 18)).any())      # the faces that are not valid give nothing ...
    assert torch.bincount(got.face)[19:].tolist() == [1, 4]               # ... a point face and a segment face do: k = 1 and the segment's k
    proper = got.face < 15
    assert _inside(got.points[proper], got.face[proper], vv, ff)
    none = geometry.surface_samples(vv, ff[:0], 1.0)
    assert none.points.shape == (0, 3) and none.face.shape == (0,) and int(none.capped) == 0


# ---- metrics ----------------------------------------------------------------------------------------------------------------------
def test_metrics_on_concentric_spheres():
    """Marching-cubes spheres of radius 6.1 and 9.6 about one centre of a 24^3 lattice (step h = 1; small, because CPU tensors run
    all pairs): every sampled distance against the analytic 3.5.  A marching-cubes vertex lies on the sphere to O(h^2 / r) (linear interpolation of the distance field along an
    edge) and a face's inside sags by as much again.  Measured here: the worst deviation of any sample, either direction, is 0.0410;
    the bound is 2 x that, 0.0820."""
    (va, fa), (vb, fb) = cases.small_sphere(6.1), cases.small_sphere(9.6)
    spacing = 1.5
    ab = geometry.closest(geometry.surface_samples(va, fa, spacing).points, vb, fb).d2.sqrt()
    ba = geometry.closest(geometry.surface_samples(vb, fb, spacing).points, va, fa).d2.sqrt()
    worst = max(float((ab - 3.5).abs().max()), float((ba - 3.5).abs().max()))
    print(f'concentric spheres: worst deviation {worst:.4f} over {len(ab) + len(ba)} samples')
    assert worst <= 0.0820
    thresholds = (3.4, 3.5, 3.6)
    g = geometry.compare(va, fa, vb, fb, spacing, thresholds)
    swapped = geometry.compare(vb, fb, va, fa, spacing, thresholds)
    assert g.forward.n == len(ab) and g.backward.n == len(ba) and g.thresholds == thresholds
    assert float(g.hausdorff) == float(swapped.hausdorff) == max(float(ab.max()), float(ba.max()))
    assert float(g.chamfer) == float(swapped.chamfer) and abs(float(g.chamfer) - 7.0) <= 2 * 0.0820
    assert torch.equal(g.precision, swapped.recall) and torch.equal(g.fscore, swapped.fscore)
    for d, direction in ((ab, g.forward), (ba, g.backward)):
        assert direction.within.dtype == torch.int64 and direction.within.tolist() == [int((d * d <= t * t).sum()) for t in thresholds]
        assert float(direction.max) == float(d.max()) and abs(float(direction.mean) - float(d.mean())) <= 1e-12 * float(d.mean())
        assert abs(float(direction.rms) - math.sqrt(float((d * d).mean()))) <= 1e-12 * float(direction.rms)
    assert g.forward.within[0] == 0 and g.forward.within[2] == g.forward.n and float(g.fscore[2]) == 1.0 and float(g.fscore[0]) == 0.0
    # a mesh against itself: default thresholds; default spacing on a tetrahedron (its faces want k = 300 and get k_max)
    own = geometry.compare(va, fa, va, fa, spacing)
    assert own.fscore.tolist() == [1.0, 1.0, 1.0] and float(own.hausdorff) < 1e-5 and own.forward.within.dtype == torch.int64
    diag = geometry.diagonal(va)
    assert own.thresholds == tuple(diag * t for t in (0.0025, 0.005, 0.01)) and abs(diag - 2 * 6.1 * math.sqrt(3)) < 0.2
    tv, tf = _t([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]), torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    tetra = geometry.compare(tv, tf, tv, tf, k_max=8)
    assert tetra.forward.n == 4 * 64 and tetra.fscore.tolist() == [1.0, 1.0, 1.0] and float(tetra.hausdorff) < 1e-7


def test_distance_stats_counts_and_one_direction():
    d2 = torch.tensor([0.0, 1.0, 4.0, 4.0, 9.0, math.inf], dtype=torch.float64)
    g = geometry.distance_stats(d2, (1.0, 2.0, 2.5))
    assert g.backward is None and g.forward.n == 6 and g.forward.within.tolist() == [2, 4, 4] and g.forward.within.dtype == torch.int64
    assert math.isinf(float(g.hausdorff)) and g.precision.tolist() == [2 / 6, 4 / 6, 4 / 6]
    finite = geometry.distance_stats(d2[:5], (3.0,), d2[:2])
    assert float(finite.forward.mean) == 8 / 5 and float(finite.forward.rms) == math.sqrt(18 / 5) and float(finite.hausdorff) == 3.0
    assert float(finite.chamfer) == 8 / 5 + 0.5 and finite.recall.tolist() == [1.0]
    empty = geometry.distance_stats(d2[:0], (1.0,))
    assert empty.forward.n == 0 and empty.forward.within.tolist() == [0] and float(empty.forward.mean) == 0.0
    for bad in ((2.0, 1.0), (-1.0,), (math.nan,), (1.0, 1.0)):
        with pytest.raises(ValueError):
            geometry.distance_stats(d2, bad)
    with pytest.raises(ValueError):
        geometry.distance_stats(d2.float(), (1.0,))


# ---- simplify_to --------------------------------------------------------------------------------------------------------------------
def test_simplify_to_keeps_its_promise():
    v, f = cases.small_sphere(6.1)
    tolerance, spacing = 0.5, 1.5
    sv, sf, cell, agreement = mesh.simplify_to(v, f, tolerance, spacing)
    rung = round(4 * math.log2(cell / (tolerance / 4)))
    assert 0 <= rung < mesh.SIMPLIFY_RUNGS and cell == tolerance / 4 * 2.0 ** (rung / 4) and len(sf) < len(f)
    pv, pf = mesh.simplify(v, f, cell)
    assert torch.equal(sv, pv) and torch.equal(sf, pf)
    measured = geometry.compare(v, f, sv, sf, spacing, (tolerance,))       # the post-condition, measured again here
    assert float(measured.hausdorff) <= tolerance and float(measured.hausdorff) == float(agreement.hausdorff)
    assert measured.forward.within.tolist() == [measured.forward.n] and measured.backward.within.tolist() == [measured.backward.n]
    above = mesh.simplify(v, f, tolerance / 4 * 2.0 ** ((rung + 1) / 4))
    assert float(geometry.compare(v, f, *above, spacing, (tolerance,)).hausdorff) > tolerance
    # a tolerance no rung can meet (its cells are finer than simplify's keys can count): the input and None
    tv, tf, tcell, tagreement = mesh.simplify_to(v, f, 1e-7, spacing)
    assert tcell is None and tagreement is None and torch.equal(tv, v) and torch.equal(tf, f)
    for bad in (0.0, -1.0, math.inf):
        with pytest.raises(ValueError):
            mesh.simplify_to(v, f, bad)


def test_pipelines_reject_cell_with_tolerance_and_defaults_do_not_move(monkeypatch):
    from pix2pix3d_amd import atlas, texture
    from test_texture_host import small_generator
    G, ws, thr = small_generator('seg2cat')
    kw = dict(resolution=32, threshold=thr, n_frames=2, image_size=64)
    for fn in (mesh.extract_mesh, texture.textured_mesh, atlas.atlas_mesh):
        with pytest.raises(ValueError, match='exclude'):
            fn(G, ws, cell=0.05, tolerance=0.01, **kw)
    v0, f0 = mesh._clean_geometry(G, ws, 32, thr, None, 1, None)
    # (tolerance= itself runs in tests/test_geometry_gpu.py: at the default spacing the all-pairs definition is no CPU test)
    # the defaults: the bytes of the stages as they were, and the new path does not run at all
    monkeypatch.setattr(mesh, 'simplify_to', None)
    monkeypatch.setattr(geometry, 'compare', None)
    base = mesh.extract_mesh(G, ws, **kw)
    labels, col = mesh.vertex_labels(G, ws, v0)
    poses, cam = mesh.script_turntable(G, 2)
    assert torch.equal(base[0], v0) and torch.equal(base[1], f0) and torch.equal(base[2], col)
    assert torch.equal(base[3], mesh.render(v0, f0, poses, cam, 64, colors=col))
    celled = mesh.extract_mesh(G, ws, cell=0.05, keep=1, **kw)
    cv, cf = mesh.simplify(*mesh.clean(v0, f0, 1)[:2], 0.05)
    cv, cf, _ = mesh.clean(cv, cf, 1)
    assert torch.equal(celled[0], cv) and torch.equal(celled[1], cf)


# ---- colours ----------------------------------------------------------------------------------------------------------------------
def test_distance_colors_table_and_buckets():
    scale = 0.37
    d = torch.cat([torch.linspace(0, 2 * scale, 1001, dtype=torch.float64), torch.tensor([math.inf, scale, scale / 255], dtype=torch.float64)])
    col = geometry.distance_colors(d * d, scale)
    assert col.dtype == torch.uint8 and col.shape == (len(d), 3)
    assert col[0].tolist() == [0, 0, 0] and col[-3].tolist() == [255, 255, 255] and col[-2].tolist() == [255, 255, 255]      # the table's ends
    assert col[-1].tolist() == [3, 0, 0] and col[1000].tolist() == [255, 255, 255]
    level = col.long().sum(1)[:1001]
    assert bool((level[1:] >= level[:-1]).all()) and len(torch.unique(level)) == 256                                       # monotone, every bucket
    grey = geometry.distance_colors(d * d, scale, 'grey')
    edges = [(scale * i / 255) ** 2 for i in range(1, 256)]
    assert grey[:, 0].tolist() == [sum(e <= x for e in edges) for x in (d * d).tolist()]
    table = torch.arange(768, dtype=torch.uint8).reshape(256, 3)
    assert torch.equal(geometry.distance_colors(d * d, scale, table), table[grey[:, 0].long()])
    for bad in (dict(scale=0.0), dict(scale=math.inf), dict(scale=1.0, palette='jet'), dict(scale=1.0, palette=table[:5])):
        with pytest.raises(ValueError):
            geometry.distance_colors(d * d, **bad)
    # a heat map of the small spheres against the large: one call each, colours for mesh.render
    v, f = three_spheres()
    near = geometry.closest(v[:50], *cases.small_sphere(9.6)).d2
    assert geometry.distance_colors(near, 5.0).shape == (50, 3)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.lib()
    names = ['p3d_mesh_bvh_build', 'p3d_mesh_bvh_keys', 'p3d_mesh_closest', 'p3d_mesh_sample_counts', 'p3d_mesh_sample_points']
    assert set(names) <= set(_lib.HEADER.functions)      # declared by the product header itself: bound when the library is loaded
    assert (geometry.K_MAX_CAP, geometry.LEAF, geometry.MAX_DEPTH, _lib.HEADER.constants['P3D_MESH_BVH_MARGIN_LOG2']) == (1024, 4, 31, 20)
    n0 = _lib.launch_count()
    for name in names:
        restype, argtypes = _lib.HEADER.functions[name]
        assert getattr(lib._handle, name).argtypes == argtypes and ctypes.c_void_p in argtypes
        code = getattr(lib, name)(*[None if t is ctypes.c_void_p else t(1) for t in argtypes])      # one face, one point, spacing^2 = 1: only the pointers are wrong
        assert code == _lib.P3D_ERR_ARGUMENT, (name, code)
        assert b'null pointer' in lib.p3d_last_error(), (name, lib.p3d_last_error())
    spare = (ctypes.c_float * 64)()
    at = ctypes.cast(spare, ctypes.c_void_p)
    assert lib.p3d_mesh_sample_counts(at, 3, at, 1, 0.0, 4, at, at, None) == _lib.P3D_ERR_ARGUMENT and b'spacing' in lib.p3d_last_error()
    assert lib.p3d_mesh_sample_counts(at, 3, at, 1, 1.0, geometry.K_MAX_CAP + 1, at, at, None) == _lib.P3D_ERR_ARGUMENT
    assert lib.p3d_mesh_sample_counts(at, 3, at, 2 ** 31 - 1, 1.0, 4, at, at, None) == _lib.P3D_ERR_UNSUPPORTED
    assert lib.p3d_mesh_bvh_build(at, 3, at, 9, at, 2, at, at, None) == _lib.P3D_ERR_ARGUMENT and b'n_pad' in lib.p3d_last_error()      # 9 faces: 3 leaves, n_pad 4
    assert lib.p3d_mesh_closest(at, 1, at, at, 9, 8, at, at, at, None) == _lib.P3D_ERR_ARGUMENT and b'n_pad' in lib.p3d_last_error()
    assert lib.p3d_mesh_closest(at, -1, at, at, 9, 4, at, at, at, None) == _lib.P3D_ERR_ARGUMENT
    assert lib.p3d_mesh_sample_points(at, 3, at, 1, at, at, 2 ** 31 - 1, at, at, None) == _lib.P3D_ERR_UNSUPPORTED
    assert _lib.launch_count() == n0
