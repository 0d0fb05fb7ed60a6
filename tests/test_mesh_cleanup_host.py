"""pix2pix3d_amd.mesh clean-up on CPU tensors: components against a plain union-find, strips and a fan with permuted ids, clean against
marching cubes of the surviving spheres alone, the properties of vertex clustering, the duplicate rule on a thin plate, argument errors
and empty meshes.  The builders here also feed tests/test_mesh_cleanup_gpu.py."""
import functools

import numpy as np
import pytest
import torch

from pix2pix3d_amd import mesh, shape
from test_shape_host import sphere

SPHERES = (((16, 16, 16), 11.3), ((36, 36, 36), 6.2), ((40, 10, 12), 2.4))


def spheres_field(which=(0, 1, 2), n=48, spheres=SPHERES):
    u = None
    for k in which:
        s = sphere(n, spheres[k][1], list(spheres[k][0]))
        u = s if u is None else torch.maximum(u, s)
    return u


@functools.lru_cache(maxsize=None)
def three_spheres():
    """(vertices, faces) of three separate closed spheres on a 48^3 lattice, index space.  Do not modify."""
    return shape.marching_cubes(spheres_field(), 0.0)


@functools.lru_cache(maxsize=None)
def plate():
    """A disc 1.6 lattice steps thick: both sides fall into the same cells at cell 2.0."""
    g = torch.stack(torch.meshgrid(*[torch.arange(40, dtype=torch.float64)] * 3, indexing='ij'), -1)
    x, y, z = g.unbind(-1)
    u = torch.minimum(0.8 - (z - 19.63).abs(), 14.2 - torch.hypot(x - 19.5, y - 19.5)).float()
    return shape.marching_cubes(u, 0.0)


def strips(n_strips, length, seed=0):
    """n_strips triangle strips of `length` triangles each, every vertex id sent through one seeded permutation: (faces, V, expected)."""
    per = length + 2
    nv = n_strips * per
    perm = torch.randperm(nv, generator=torch.Generator().manual_seed(seed))
    i = torch.arange(length)
    base = (torch.arange(n_strips) * per)[:, None, None]
    faces = (base + torch.stack([i, i + 1, i + 2], -1)[None]).reshape(-1, 3)
    expected = torch.empty([nv], dtype=torch.int64)
    expected[perm] = perm.view(n_strips, per).min(1).values.repeat_interleave(per)
    return perm[faces], nv, expected


def fan(ring):
    """One hub with the LARGEST id joined to a ring: every hook of a naive scheme lands on one parent word."""
    i = torch.arange(ring)
    return torch.stack([torch.full_like(i, ring), i, (i + 1) % ring], -1), ring + 1


def union_find(faces, nv):
    """Plain-Python union-find with full compression at the end; labels = the smallest id of each set."""
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in faces.tolist():
        for p, q in ((a, b), (b, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)
    return torch.tensor([find(v) for v in range(nv)], dtype=torch.int64)


def euler(nv_used, faces):
    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).sort(1).values
    return nv_used - len(torch.unique(e, dim=0)) + len(faces)


# ---- components ---------------------------------------------------------------------------------------------
def test_three_spheres_are_what_the_tests_assume():
    v, f = three_spheres()
    assert (len(v), len(f)) == (3258, 6504)
    label = union_find(f, len(v))
    roots, counts = torch.unique(label[f[:, 0]], return_counts=True)
    assert sorted(counts.tolist(), reverse=True) == [4808, 1448, 248]
    for r in roots:
        part = f[label[f[:, 0]] == r]
        assert euler(len(torch.unique(part)), part) == 2


def test_components_match_union_find():
    v, f = three_spheres()
    ref = union_find(f, len(v))
    got = mesh.components(f, len(v))
    assert got.dtype == torch.int64 and torch.equal(got, ref)
    g = torch.Generator().manual_seed(3)
    assert torch.equal(mesh.components(f[torch.randperm(len(f), generator=g)], len(v)), ref)         # face order does not matter
    assert torch.equal(mesh.components(f.to(torch.int32), len(v)), ref)
    perm = torch.randperm(len(v), generator=g)                                                      # old id -> new id
    moved = mesh.components(perm[f], len(v))
    assert torch.equal(moved, union_find(perm[f], len(v)))
    # the same partition: the new label of perm[v] is the smallest new id among the old component of v
    smallest = torch.full([len(v)], len(v), dtype=torch.int64).scatter_reduce_(0, ref, perm, 'amin')
    assert torch.equal(moved[perm], smallest[ref])


@pytest.mark.parametrize('n_strips,length', [(1, 100_000), (1000, 100)])
def test_components_strips_with_permuted_ids(n_strips, length):
    faces, nv, expected = strips(n_strips, length)
    assert torch.equal(mesh.components(faces, nv), expected)


def test_components_fan_with_the_hub_last():
    faces, nv = fan(50_000)
    assert torch.equal(mesh.components(faces, nv), torch.zeros([nv], dtype=torch.int64))


def test_components_unused_vertices_are_their_own():
    faces = torch.tensor([[5, 2, 7], [7, 9, 2]])
    assert mesh.components(faces, 11).tolist() == [0, 1, 2, 3, 4, 2, 6, 2, 8, 2, 10]


# ---- clean ----------------------------------------------------------------------------------------------------
def _assert_same_mesh(got, want):
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))                         # vertices bit for bit
    assert got[1].dtype == torch.int64 and torch.equal(got[1], want[1])


def test_clean_keeps_the_largest_spheres():
    v, f = three_spheres()
    big = shape.marching_cubes(spheres_field((0,)), 0.0)
    two = shape.marching_cubes(spheres_field((0, 1)), 0.0)
    for keep, want in ((1, big), (2, two), (3, (v, f)), (7, (v, f)), (None, (v, f))):
        cv, cf, kept = mesh.clean(v, f, keep=keep)
        _assert_same_mesh((cv, cf), want)
        assert kept.dtype == torch.int64 and torch.equal(v[kept], cv)
        assert bool((kept[1:] > kept[:-1]).all())
    assert len(big[1]) == 4808 and len(two[1]) == 4808 + 1448


def test_clean_min_faces():
    v, f = three_spheres()
    two = shape.marching_cubes(spheres_field((0, 1)), 0.0)
    _assert_same_mesh(mesh.clean(v, f, keep=None, min_faces=248)[:2], (v, f))                       # the smallest has exactly 248
    _assert_same_mesh(mesh.clean(v, f, keep=None, min_faces=249)[:2], two)                          # ... and goes at 249, alone
    _assert_same_mesh(mesh.clean(v, f, keep=1, min_faces=249)[:2], shape.marching_cubes(spheres_field((0,)), 0.0))
    cv, cf, kept = mesh.clean(v, f, keep=None, min_faces=4809)                                      # more than the largest: nothing is left
    assert cv.shape == (0, 3) and cf.shape == (0, 3) and kept.shape == (0,)
    cv, cf, kept = mesh.clean(v, f, keep=2, min_faces=1449)                                         # keep counts only those that pass
    assert len(cf) == 4808


def test_clean_tie_goes_to_the_smaller_label():
    twins = (((12.3, 12.1, 12.2), 6.2), ((32.3, 12.1, 12.2), 6.2))                                   # one sphere and its copy 20 steps along x
    v, f = shape.marching_cubes(spheres_field((0, 1), spheres=twins), 0.0)
    first = shape.marching_cubes(spheres_field((0,), spheres=twins), 0.0)
    assert len(f) == 2 * len(first[1])
    cv, cf, kept = mesh.clean(v, f, keep=1)
    _assert_same_mesh((cv, cf), first)
    assert int(kept[0]) == 0


# ---- simplify -------------------------------------------------------------------------------------------------
def cell_of_vertices(v, cell):
    """The test's own statement of the cell rule: (cluster id of every vertex, integer cell coordinates of every cluster, lo)."""
    lo = v.min(0).values.double().numpy()
    i = np.floor((v.double().numpy() - lo) / float(cell)).astype(np.int64)
    n = i.max(0) + 1
    key = (i[:, 2] * n[1] + i[:, 1]) * n[0] + i[:, 0]
    uniq, inverse = np.unique(key, return_inverse=True)
    coords = np.stack([uniq % n[0], uniq // n[0] % n[1], uniq // (n[0] * n[1])], -1)
    return torch.from_numpy(inverse.reshape(-1)), coords, lo


def check_simplified(v, f, cell, sv, sf):
    """Every property of the issue for one (mesh, cell, result); returns the number of non-degenerate input faces."""
    cluster, coords, lo = cell_of_vertices(v, cell)
    assert sv.dtype == torch.float32 and sf.dtype == torch.int64
    assert len(sv) == len(coords)                                                                    # one vertex per occupied cell
    box_lo = lo + coords * float(cell)
    slack = 1e-5 * float(cell)
    assert (sv.double().numpy() >= box_lo - slack).all() and (sv.double().numpy() <= box_lo + float(cell) + slack).all()
    mean = torch.zeros([len(coords), 3], dtype=torch.float64).index_add_(0, cluster, v.double())
    mean /= torch.bincount(cluster).double()[:, None]
    assert (sv.double() - mean).abs().max() <= 2.0 ** -23 * float(v.abs().max())                    # the mean, to one fp32 rounding
    srt = sf.sort(1).values
    assert bool((srt[:, 0] < srt[:, 1]).all() and (srt[:, 1] < srt[:, 2]).all())                    # no repeated index
    assert len(torch.unique(srt, dim=0)) == len(sf)                                                  # no two faces share a vertex set
    mapped = cluster[f]
    first = {}
    n_live = 0
    for t, row in enumerate(mapped.tolist()):
        if len(set(row)) == 3:
            n_live += 1
            first.setdefault(tuple(sorted(row)), t)
    where = [first[tuple(r)] for r in srt.tolist()]                                                  # KeyError: a face that was never there
    assert len(where) == len(first)
    assert all(a < b for a, b in zip(where, where[1:]))                                             # a subsequence of the input order
    assert torch.equal(sf, mapped[torch.tensor(where, dtype=torch.int64)])                          # each with the first one's winding
    return n_live


@pytest.mark.parametrize('cell,n_faces', [(1.0, 3906), (2.0, 1314), (4.0, 358)])
def test_simplify_three_spheres(cell, n_faces):
    v, f = three_spheres()
    sv, sf = mesh.simplify(v, f, cell)
    check_simplified(v, f, cell, sv, sf)
    assert len(sf) == n_faces
    assert len(sf) < len(f)


def test_simplify_cell_below_the_shortest_edge_changes_nothing():
    v, f = three_spheres()
    e = torch.cat([v[f[:, 0]] - v[f[:, 1]], v[f[:, 1]] - v[f[:, 2]], v[f[:, 2]] - v[f[:, 0]]]).double().norm(dim=1)
    cell = float(e.min()) * 0.5
    cluster, coords, _ = cell_of_vertices(v, cell)
    assert len(coords) == len(v)                                                                     # no two vertices share a cell
    sv, sf = mesh.simplify(v, f, cell)
    assert len(sf) == len(f)
    rows = lambda t: sorted(map(tuple, t.tolist()))                                                  # noqa: E731
    assert rows(sv) == rows(v)
    assert torch.equal(sv[sf], v[f])                                                                 # the same triangles, in order, renumbered


def test_simplify_thin_plate_becomes_single_sided():
    v, f = plate()
    sv, sf = mesh.simplify(v, f, 2.0)
    n_live = check_simplified(v, f, 2.0, sv, sf)
    assert n_live >= 300
    assert len(sf) <= n_live * 2 / 3, (n_live, len(sf))                                              # matching up to rotation only would remove none


# ---- errors and empty meshes ----------------------------------------------------------------------------------
def test_argument_errors():
    v, f = three_spheres()
    bad = f.clone()
    bad[17, 1] = len(v)
    neg = f.clone()
    neg[0, 0] = -1
    for faces in (bad, neg):
        with pytest.raises(ValueError):
            mesh.components(faces, len(v))
        with pytest.raises(ValueError):
            mesh.clean(v, faces)
        with pytest.raises(ValueError):
            mesh.simplify(v, faces, 2.0)
    for value in (float('nan'), float('inf')):
        w = v.clone()
        w[5, 2] = value
        with pytest.raises(ValueError):
            mesh.clean(w, f)
        with pytest.raises(ValueError):
            mesh.simplify(w, f, 2.0)
    for cell in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            mesh.simplify(v, f, cell)
    for keep in (0, -3):
        with pytest.raises(ValueError):
            mesh.clean(v, f, keep=keep)
    with pytest.raises(ValueError):
        mesh.components(f[:, :2], len(v))
    with pytest.raises(ValueError):
        mesh.simplify(v, f, 1e-30)                                                                   # more cells than a key holds


def test_empty_meshes_pass_through():
    none = torch.empty([0, 3], dtype=torch.int64)
    assert torch.equal(mesh.components(none, 5), torch.arange(5))
    assert mesh.components(none, 0).shape == (0,)
    v = three_spheres()[0]
    cv, cf, kept = mesh.clean(v, none)
    assert cv.shape == (0, 3) and cf.shape == (0, 3) and kept.shape == (0,) and cf.dtype == torch.int64
    sv, sf = mesh.simplify(v, none, 4.0)
    assert sf.shape == (0, 3) and sf.dtype == torch.int64 and len(sv) == len(cell_of_vertices(v, 4.0)[1])
    nothing = torch.empty([0, 3])
    cv, cf, kept = mesh.clean(nothing, none)
    assert cv.shape == (0, 3) and cf.shape == (0, 3) and kept.shape == (0,)
    sv, sf = mesh.simplify(nothing, none, 1.0)
    assert sv.shape == (0, 3) and sf.shape == (0, 3)
