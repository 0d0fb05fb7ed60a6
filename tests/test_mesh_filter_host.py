"""pix2pix3d_amd.mesh filtering on CPU tensors, where the formulation is the definition: the adjacency lists and boundary flags, what
Taubin smoothing does to a noisy sphere (and what plain Laplacian smoothing does instead), pinning, the invariants of a step, the
majority vote on speckled labels and its tie rule, smooth shading against a closed form and against the flat shade, and the defaults of
the pipelines.  The builders here also feed tests/test_mesh_filter_gpu.py."""
import functools
import math

import pytest
import torch

from pix2pix3d_amd import mesh, shape, texture
from test_mesh_cleanup_host import fan, three_spheres
from test_shape_host import sphere

CENTRE = (23.4, 24.1, 23.7)


@functools.lru_cache(maxsize=None)
def open_sphere():
    """A sphere the lattice cuts at z = 0: an open mesh with one rim.  Do not modify."""
    return shape.marching_cubes(sphere(32, 14.0, [16, 16, 4]), 0.0)


@functools.lru_cache(maxsize=None)
def noisy_sphere():
    """(clean vertices, noisy vertices, faces) of a sphere of radius 17.3 about CENTRE, noise 0.3 randn with seed 0.  Do not modify."""
    v, f = shape.marching_cubes(sphere(48, 17.3, list(CENTRE)), 0.0)
    return v, v + 0.3 * torch.randn(v.shape, generator=torch.Generator().manual_seed(0)), f


@functools.lru_cache(maxsize=None)
def speckled_labels():
    """(truth, speckled) labels on the sphere: four quadrants, 5 % of the vertices redrawn from 6 labels with seed 1.  Do not modify."""
    v, _, _ = noisy_sphere()
    truth = (v[:, 0] > CENTRE[0]).long() + 2 * (v[:, 1] > CENTRE[1]).long()
    g = torch.Generator().manual_seed(1)
    pick = torch.rand(len(v), generator=g) < 0.05
    return truth, torch.where(pick, torch.randint(0, 6, [len(v)], generator=g), truth)


def lists(adj):
    return [adj.neighbours[adj.offsets[v]:adj.offsets[v + 1]].tolist() for v in range(len(adj.boundary))]


def same_bits(a, b):
    return a.dtype == b.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def volume(v, f):
    p = v.double()[f]
    return float((p[:, 0] * torch.linalg.cross(p[:, 1], p[:, 2])).sum() / 6)


# ---- adjacency ----------------------------------------------------------------------------------------------------------------
def test_adjacency_of_a_closed_mesh():
    v, f = three_spheres()
    adj = mesh.adjacency(f, len(v))
    assert adj.offsets.dtype == torch.int64 and adj.neighbours.dtype == torch.int32 and adj.boundary.dtype == torch.bool
    assert tuple(adj.offsets.shape) == (len(v) + 1,) and int(adj.offsets[0]) == 0 and int(adj.offsets[-1]) == len(adj.neighbours)
    nb = lists(adj)
    for a, row in enumerate(nb):
        assert row == sorted(set(row)) and a not in row
        assert all(a in nb[b] for b in row)                                 # symmetric
    want = [set() for _ in range(len(v))]
    for a, b, c in f.tolist():
        want[a] |= {b, c}; want[b] |= {a, c}; want[c] |= {a, b}
    assert [set(row) for row in nb] == want
    degree = adj.offsets[1:] - adj.offsets[:-1]
    assert int(degree.min()) == 4 and int(degree.max()) == 10
    assert not adj.boundary.any()


def test_adjacency_of_an_open_mesh_flags_the_rim():
    v, f = open_sphere()
    adj = mesh.adjacency(f, len(v))
    assert len(v) == 2361 and int(adj.boundary.sum()) == 108
    assert (v[adj.boundary][:, 2] == 0).all()


def test_adjacency_does_not_depend_on_face_or_corner_order():
    v, f = open_sphere()
    adj = mesh.adjacency(f, len(v))
    for other in (f.flip(0), f[:, [1, 2, 0]], f.flip(0)[:, [2, 0, 1]], f.int()):
        got = mesh.adjacency(other, len(v))
        assert all(torch.equal(a, b) for a, b in zip(adj, got))


def test_adjacency_edge_cases():
    # a closed tetrahedron on 0..3, a face with a repeated index that joins 1 and 4, and vertex 5 that no face uses
    faces = torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2], [4, 1, 4]])
    adj = mesh.adjacency(faces, 6)
    assert lists(adj) == [[1, 2, 3], [0, 2, 3, 4], [0, 1, 3], [0, 1, 2], [1], []]
    assert not adj.boundary.any()                                          # the degenerate face flags nothing by itself
    assert mesh.adjacency(torch.tensor([[2, 2, 2]]), 3).neighbours.numel() == 0
    one = mesh.adjacency(torch.tensor([[0, 1, 2]]), 4)
    assert one.boundary.tolist() == [True, True, True, False]
    # an edge three faces share is not a boundary edge: the fins' other edges are
    fins = mesh.adjacency(torch.tensor([[0, 1, 2], [0, 1, 3], [0, 1, 4]]), 5)
    assert fins.boundary.all() and lists(fins)[0] == [1, 2, 3, 4]
    closed = torch.tensor([[0, 1, 2], [1, 0, 2]])                          # both sides of one triangle: every edge twice
    assert not mesh.adjacency(closed, 3).boundary.any()
    empty = mesh.adjacency(torch.zeros([0, 3], dtype=torch.int64), 2)
    assert empty.offsets.tolist() == [0, 0, 0] and empty.neighbours.numel() == 0 and not empty.boundary.any()
    with pytest.raises(ValueError, match='face index'):
        mesh.adjacency(torch.tensor([[0, 1, 3]]), 3)


# ---- smoothing ----------------------------------------------------------------------------------------------------------------
def test_taubin_smooths_a_noisy_sphere_and_keeps_its_volume():
    """Measured with this formulation: the std of the radii 0.303 -> 0.118, the volume +0.08 %; ten Laplacian steps alone -2.3 %."""
    _, noisy, f = noisy_sphere()
    assert len(noisy) == 5626
    centre = torch.tensor(CENTRE)
    out = mesh.smooth(noisy, f)
    assert out.dtype == torch.float32 and out.shape == noisy.shape
    before, after = float((noisy - centre).norm(dim=1).std()), float((out - centre).norm(dim=1).std())
    print(f'radius std {before:.4f} -> {after:.4f}')
    assert after <= 0.5 * before
    v0, v1 = volume(noisy, f), volume(out, f)
    print(f'volume {v1 / v0 - 1:+.5f}')
    assert abs(v1 / v0 - 1) <= 0.005
    laplace = volume(mesh.smooth(noisy, f, mu=0), f)
    print(f'volume, mu = 0: {laplace / v0 - 1:+.5f}')
    assert laplace / v0 - 1 < -0.01                                        # why mu exists


def test_smooth_is_the_stated_arithmetic():
    """One step against a plain-Python walk of the lists in Python floats (fp64, one rounding per operation)."""
    v, f = open_sphere()
    adj = mesh.adjacency(f, len(v))
    got = mesh.smooth(v, f, iterations=1, lam=0.37, mu=0, pin_boundary=False)
    rows = v.double().tolist()
    want = []
    for a, nb in enumerate(lists(adj)):
        out = []
        for c in range(3):
            acc = 0.0
            for w in nb:
                acc = acc + rows[w][c]
            out.append(rows[a][c] + 0.37 * (acc / len(nb) - rows[a][c]))
        want.append(out)
    assert same_bits(got, torch.tensor(want, dtype=torch.float64).float())


def test_pinning_the_boundary():
    v, f = open_sphere()
    adj = mesh.adjacency(f, len(v))
    out = mesh.smooth(v, f)
    moved = (out.view(torch.int32) != v.view(torch.int32)).any(1)
    assert not moved[adj.boundary].any() and int(moved.sum()) == 2253
    free = mesh.smooth(v, f, pin_boundary=False)
    assert (free.view(torch.int32) != v.view(torch.int32)).any(1)[adj.boundary].any()
    mask = torch.zeros(len(v), dtype=torch.bool)
    mask[::3] = True
    out = mesh.smooth(v, f, pinned=mask, adjacency=adj)
    assert same_bits(out[mask | adj.boundary], v[mask | adj.boundary])


def test_smoothing_invariants():
    v, f = open_sphere()
    assert same_bits(mesh.smooth(v, f, iterations=0), v)
    assert same_bits(mesh.smooth(v, f, pinned=torch.ones(len(v), dtype=torch.bool)), v)
    lonely = torch.cat([v, torch.tensor([[1.5, 2.5, 3.5]])])               # a vertex no face uses
    out = mesh.smooth(lonely, f, iterations=3)
    assert same_bits(out[-1:], lonely[-1:]) and same_bits(out[:-1], mesh.smooth(v, f, iterations=3))
    assert same_bits(mesh.smooth(v, f.flip(0)[:, [1, 2, 0]], iterations=3), mesh.smooth(v, f, iterations=3))
    assert same_bits(mesh.smooth(v, None, iterations=3, adjacency=mesh.adjacency(f, len(v))), mesh.smooth(v, f, iterations=3))
    empty = mesh.smooth(torch.zeros([0, 3]), torch.zeros([0, 3], dtype=torch.int64))
    assert tuple(empty.shape) == (0, 3)


def test_the_long_list_of_a_fan_sums_in_list_order():
    faces, nv = fan(3000)
    x = torch.rand([nv, 3], generator=torch.Generator().manual_seed(5)) * 100
    got = mesh.smooth(x, faces, iterations=1, lam=1.0, mu=0, pin_boundary=False)
    rows = x.double().tolist()
    want = []
    for c in range(3):
        acc = 0.0
        for w in range(nv - 1):
            acc = acc + rows[w][c]
        want.append(rows[-1][c] + 1.0 * (acc / (nv - 1) - rows[-1][c]))
    assert same_bits(got[-1], torch.tensor(want, dtype=torch.float64).float())


def test_smooth_argument_errors():
    v, f = open_sphere()
    for bad in (dict(lam=0.0), dict(lam=1.5), dict(lam=-0.5), dict(mu=-0.5), dict(mu=0.2), dict(mu=float('nan')), dict(lam=float('nan')),
                dict(iterations=-1), dict(iterations=1.5)):
        with pytest.raises(ValueError, match='smooth'):
            mesh.smooth(v, f, **bad)
    assert mesh.smooth(v, f, iterations=1, lam=1.0, mu=-1.01).shape == v.shape
    broken = v.clone()
    broken[7, 1] = float('inf')
    with pytest.raises(ValueError, match='finite'):
        mesh.smooth(broken, f)
    with pytest.raises(ValueError, match='pinned'):
        mesh.smooth(v, f, pinned=torch.ones(len(v) - 1, dtype=torch.bool))
    with pytest.raises(ValueError, match='adjacency'):
        mesh.smooth(v, f, adjacency=mesh.adjacency(f, len(v) + 1))
    with pytest.raises(ValueError, match='face index'):
        mesh.smooth(v[:-1], f)


def test_smooth_values_types_and_rounding():
    v, f = three_spheres()
    g = torch.Generator().manual_seed(3)
    colours = torch.randint(0, 256, [len(v), 3], generator=g, dtype=torch.uint8)
    out = mesh.smooth_values(colours, f, iterations=2)
    assert out.dtype == torch.uint8 and out.shape == colours.shape
    step = mesh.smooth_values(colours.float(), f, iterations=2)
    assert step.dtype == torch.float32 and torch.equal(out, torch.floor(step + 0.5).clamp(0, 255).to(torch.uint8))
    assert float(out.float().std()) < 0.6 * float(colours.float().std())
    constant = torch.full([len(v), 4], 37, dtype=torch.uint8)
    assert torch.equal(mesh.smooth_values(constant, f, iterations=3), constant)
    assert torch.equal(mesh.smooth_values(colours, f, iterations=0), colours)
    wide = torch.rand([len(v), 7], generator=g)
    one = mesh.smooth_values(wide, f)
    for c in (0, 6):                                                        # channels are independent
        assert same_bits(one[:, c:c + 1], mesh.smooth_values(wide[:, c:c + 1].contiguous(), f))
    for bad in (torch.zeros([len(v)]), torch.zeros([len(v), 257]), torch.zeros([len(v), 0]), torch.zeros([len(v), 3], dtype=torch.float64)):
        with pytest.raises(ValueError, match='smooth_values'):
            mesh.smooth_values(bad, f)
    with pytest.raises(ValueError, match='factor'):
        mesh.smooth_values(wide, f, factor=float('inf'))


# ---- label voting ---------------------------------------------------------------------------------------------------------------
def test_label_vote_removes_speckle():
    """Measured: 235 wrong labels before, 4 after two steps."""
    _, _, f = noisy_sphere()
    truth, speckled = speckled_labels()
    assert int((speckled != truth).sum()) == 235
    out = mesh.smooth_labels(speckled, f, iterations=2)
    assert out.dtype == torch.int64 and out.shape == truth.shape
    wrong = int((out != truth).sum())
    print(f'wrong labels 235 -> {wrong}')
    assert wrong <= 10


def test_label_vote_leaves_a_clean_labelling_alone():
    _, _, f = noisy_sphere()
    truth, _ = speckled_labels()
    assert torch.equal(mesh.smooth_labels(truth, f, iterations=2), truth)   # measured: 0 changes
    assert torch.equal(mesh.smooth_labels(truth, f, iterations=0), truth)


def test_label_vote_tie_rule():
    # a fan: hub 0 joined to the ring 1, 2, 3, 4
    faces = torch.tensor([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]])
    vote = lambda labels, **kw: mesh.smooth_labels(torch.tensor(labels), faces, **kw).tolist()      # noqa: E731
    # hub: counts {5: 1 (itself), 3: 2, 1: 2} -> the smallest label that reaches the maximum; ring vertices see three labels once or
    # their own twice
    assert vote([5, 3, 3, 1, 1])[0] == 1
    # hub: counts {3: 1 + 1, 1: 2, 2: 1}: its own label reaches the maximum, so it stays, though 1 is smaller
    assert vote([3, 3, 1, 1, 2])[0] == 3
    # all different: every count is 1, everybody keeps their own
    assert vote([4, 3, 2, 1, 0]) == [4, 3, 2, 1, 0]
    # vertex 1 (neighbours 0, 2, 4) has counts {0: 1 (itself), 7: 3}: it joins them, unless it is pinned
    assert vote([7, 0, 7, 7, 7]) == [7, 7, 7, 7, 7]
    assert vote([7, 0, 7, 7, 7], pinned=torch.tensor([False, True, False, False, False])) == [7, 0, 7, 7, 7]
    # synchronous: both ends of a 0/1 pattern read the OLD labels
    assert vote([0, 1, 0, 1, 0], iterations=1) == [0, 0, 0, 0, 0]
    with pytest.raises(ValueError, match='label outside'):
        vote([0, 1, 2, 3, 6], n_labels=6)
    with pytest.raises(ValueError, match='label outside'):
        vote([0, 1, 2, 3, -1])
    with pytest.raises(ValueError, match='n_labels'):
        vote([0, 1, 2, 3, 4], n_labels=257)
    with pytest.raises(ValueError, match='labels must be'):
        mesh.smooth_labels(torch.zeros([5]), faces)
    assert vote([255, 255, 3, 255, 255]) == [255, 255, 255, 255, 255]
    lonely = mesh.smooth_labels(torch.tensor([1, 1, 1, 1, 1, 4]), faces)   # vertex 5 has no neighbours
    assert lonely.tolist() == [1, 1, 1, 1, 1, 4]


def test_label_vote_against_a_plain_count():
    v, f = three_spheres()
    adj = mesh.adjacency(f, len(v))
    labels = torch.randint(0, 6, [len(v)], generator=torch.Generator().manual_seed(2))
    got = mesh.smooth_labels(labels, f, n_labels=6)
    old = labels.tolist()
    for a, nb in enumerate(lists(adj)):
        count = [0] * 6
        count[old[a]] += 1
        for w in nb:
            count[old[w]] += 1
        want = old[a] if count[old[a]] == max(count) else count.index(max(count))
        assert int(got[a]) == want
    assert not torch.equal(got, labels)
    hub_faces, nv = fan(300)                                                # a long list: the hub sees 300 labels
    ring = torch.randint(0, 256, [nv], generator=torch.Generator().manual_seed(4))
    ring[:40] = 201
    out = mesh.smooth_labels(ring, hub_faces, n_labels=256)
    assert int(out[-1]) == 201


# ---- smooth shading -------------------------------------------------------------------------------------------------------------
def _ball():
    v, f = shape.marching_cubes(sphere(24, 8.5), 0.0)
    return v / 23 - 0.5, f


def test_smooth_shade_with_one_normal_everywhere_is_one_grey():
    v, f = _ball()
    poses = mesh.turntable_poses([0, 0, 0], 1.0, 3, yaw_range=1.0, pitch_range=0.6)
    cam = mesh.Orthographic(0.5, 0.5)
    n0 = torch.tensor([0.3, -0.5, 0.8])
    ambient = 0.25
    frames, fid, _ = mesh.render(v, f, poses, cam, 64, ambient=ambient, normals=n0.expand(len(v), 3).contiguous(), return_buffers=True)
    amb = float(torch.tensor(ambient, dtype=torch.float32))
    for k in range(3):
        fwd = poses[k, :3, 2].double()
        cosv = abs(float(n0.double() @ fwd)) / (float(n0.double().norm()) * float(fwd.norm()))
        grey = math.floor(200 * (amb + (1 - amb) * cosv) + 0.5)
        drawn = fid[k] >= 0
        assert int(drawn.sum()) > 500
        assert (frames[k][drawn] == grey).all() and (frames[k][~drawn] == 255).all()
    flat = mesh.render(v, f, poses, cam, 64, ambient=ambient)
    assert not torch.equal(flat, frames)


def test_smooth_shade_with_the_face_normal_is_the_flat_shade():
    # corners on a grid of eighths: the cross product is exact in fp32
    v = torch.tensor([[-0.25, -0.25, 0.0], [0.25, -0.25, 0.125], [0.0, 0.25, 0.0]])
    f = torch.tensor([[0, 1, 2]])
    normal = torch.linalg.cross(v[1] - v[0], v[2] - v[0])
    colors = torch.tensor([[255, 0, 0], [0, 255, 0], [10, 20, 255]], dtype=torch.uint8)
    poses = mesh.turntable_poses([0, 0, 0], 1.0, 4, yaw_range=0.8, pitch_range=0.5)
    for cam in (mesh.Orthographic(0.4, 0.4), mesh.Pinhole(torch.tensor([[2.0, 0, 0.5], [0, 2.0, 0.5], [0, 0, 1]]))):
        proj = mesh.project(v, poses, cam, 48)
        fid, _ = mesh.rasterize(proj, f, 48)
        assert int((fid >= 0).sum()) > 200
        for col in (colors, None):
            flat = mesh.shade(fid, proj, v, f, poses, col)
            smooth = mesh.shade(fid, proj, v, f, poses, col, normals=normal.expand(3, 3).contiguous())
            assert torch.equal(flat, smooth)


def test_smooth_shade_follows_the_vertex_normals():
    """With ``texture.vertex_normals`` a coarse ball loses its facets: neighbouring drawn pixels differ by less than under flat shading."""
    v, f = _ball()
    poses = mesh.turntable_poses([0, 0, 0], 1.0, 1)
    cam = mesh.Orthographic(0.45, 0.45)
    normals = texture.vertex_normals(v, f)
    flat, fid, _ = mesh.render(v, f, poses, cam, 96, return_buffers=True)
    smooth = mesh.render(v, f, poses, cam, 96, normals=normals)
    both = (fid[0, :, 1:] >= 0) & (fid[0, :, :-1] >= 0)
    jump = lambda img: (img[0, :, 1:, 0].int() - img[0, :, :-1, 0].int()).abs()[both].float()      # noqa: E731
    assert float(jump(smooth).max()) < float(jump(flat).max()) and float(jump(smooth).mean()) < float(jump(flat).mean())
    assert torch.equal((smooth == 255).all(-1), (flat == 255).all(-1))     # the same pixels are drawn


def test_shade_normals_argument_errors():
    v, f = _ball()
    poses = mesh.turntable_poses([0, 0, 0], 1.0, 1)
    proj = mesh.project(v, poses, mesh.Orthographic(0.5, 0.5), 16)
    fid, _ = mesh.rasterize(proj, f, 16)
    for bad in (torch.zeros([len(v), 3], dtype=torch.float64), torch.zeros([len(v) - 1, 3]), torch.zeros([len(v), 4]), torch.zeros([len(v) * 3])):
        with pytest.raises(ValueError, match='normals'):
            mesh.shade(fid, proj, v, f, poses, normals=bad)
        with pytest.raises(ValueError, match='normals'):
            mesh.render(v, f, poses, mesh.Orthographic(0.5, 0.5), 16, normals=bad)


# ---- the pipelines ----------------------------------------------------------------------------------------------------------------
def test_extract_mesh_defaults_are_unchanged_and_the_filters_apply():
    from test_texture_host import small_generator
    G, ws, thr = small_generator('seg2cat')
    kw = dict(resolution=32, threshold=thr, n_frames=2, image_size=64, keep=1)
    base = mesh.extract_mesh(G, ws, **kw)
    same = mesh.extract_mesh(G, ws, smooth=0, smooth_labels=0, smooth_shading=False, lam=0.5, mu=-0.53, **kw)
    assert all(torch.equal(a, b) for a, b in zip(base, same))
    # what the parent computed, stage by stage
    v, f = mesh._clean_geometry(G, ws, 32, thr, 1, 1, None)
    labels, colors = mesh.vertex_labels(G, ws, v)
    poses, cam = mesh.script_turntable(G, 2)
    assert torch.equal(base[0], v) and torch.equal(base[1], f) and torch.equal(base[2], colors)
    assert torch.equal(base[3], mesh.render(v, f, poses, cam, 64, colors=colors))
    sv, sf, scol, sframes = mesh.extract_mesh(G, ws, smooth=3, smooth_labels=2, smooth_shading=True, **kw)
    assert torch.equal(sf, f)
    assert same_bits(sv, mesh.smooth(v, f, 3))
    voted = mesh.smooth_labels(labels, f, 2, n_labels=int(G.semantic_channels))
    assert torch.equal(scol, mesh.default_palette(int(G.semantic_channels))[voted])
    assert torch.equal(sframes, mesh.render(sv, sf, poses, cam, 64, colors=scol, normals=texture.vertex_normals(sv, sf)))
    assert not torch.equal(sframes, base[3]) and not (sframes == 255).all()
