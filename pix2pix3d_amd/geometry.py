"""Geometry agreement: how far one mesh lies from another (the role of ``trimesh.proximity`` and of Metro-style sampled distances for a
user of applications/extract_mesh.py).  Every stage of the mesh pipeline (``mesh.clean``, ``mesh.simplify``, ``mesh.smooth``, a coarser
lattice, an edit of the label map) moves the surface; this module says by how much.

* ``surface_samples``: a deterministic, integer-decided point set on a mesh, dense enough that no point of a face lies farther than
  about ``spacing`` from a sample.
* ``closest`` / ``build_bvh``: per point the squared distance to the nearest triangle and that triangle's id.  CPU tensors run the
  definition, all pairs in chunks; device tensors find the same minimum, bit for bit, through a bounding-volume hierarchy
  (csrc/mesh_distance.hip).
* ``distance_stats`` / ``compare``: mean, RMS, maximum (the sampled one-sided Hausdorff distance) and counts within thresholds for one
  direction; symmetric Hausdorff, Chamfer and precision / recall / F-score for two.  Torch ops on the d2 vector: no kernel.
* ``distance_colors``: a heat map of distances as vertex colours for ``mesh.render(colors=)``, ``mesh.write_ply`` and ``atlas``.
* ``change_map``: where in 3D two latents' shapes differ, e.g. before and after an edit of the label map.
* ``mesh.simplify_to`` (in mesh.py) picks ``simplify``'s cell from a tolerance with ``compare``.

The rules (validity of a face, the subdivision count, the order of the samples, the point-to-triangle distance operation by operation,
the keys, the tree and why pruning is exact) are include/p3d_hip.h's ("mesh distances"); the CPU formulations below are the definition and the
kernels' bytes equal them.  Meshes are what ``mesh`` takes: vertices float32 [V, 3], faces int32 or int64 [T, 3], V and T below
2^31 - 1.  Unlike ``mesh.clean`` and its kin nothing here rejects a bad face: a face with an index outside [0, V) or a non-finite
corner contributes no sample and has distance +inf."""
import math
from typing import NamedTuple, Optional

import torch

from . import _lib, mesh, shape

K_MAX_CAP = _lib.HEADER.constants['P3D_MESH_SAMPLE_KMAX']
LEAF = _lib.HEADER.constants['P3D_MESH_BVH_LEAF']
MAX_DEPTH = _lib.HEADER.constants['P3D_MESH_BVH_MAX_DEPTH']
SORT_QUERIES_FROM = 1 << 14       # closest(sort_queries=None) sorts the query points by Morton key from this many points on


# ---- operands ---------------------------------------------------------------------------------------------------------------
def _mesh(what, vertices, faces):
    """(vertices float32 [V, 3] contiguous, faces int32 [T, 3] on the vertices' device): shapes and types only.  An int64 index
    outside [0, V) becomes -1, so that it cannot wrap into the range."""
    vertices = mesh._vertices32(what, vertices)
    mesh._faces32(faces)
    faces = faces.detach().to(vertices.device)
    if faces.dtype == torch.int64:
        faces = torch.where((faces < 0) | (faces >= vertices.shape[0]), torch.full_like(faces, -1), faces)
    return vertices, faces.to(torch.int32).contiguous()


def _points(what, points, device=None):
    points = torch.as_tensor(points).detach().to(torch.float32)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f'{what}: points must be [N, 3], got {tuple(points.shape)}')
    return (points if device is None else points.to(device)).contiguous()


def _corners(vertices, faces32):
    """(valid bool [T], corners float64 [T, 3 corners, 3]) with zeros where the face is not valid."""
    nv, idx = vertices.shape[0], faces32.long()
    ok = ((idx >= 0) & (idx < nv)).all(1)
    if nv == 0:
        return ok, torch.zeros([idx.shape[0], 3, 3], dtype=torch.float64, device=vertices.device)
    corners = vertices.double()[idx.clamp(0, nv - 1)]
    ok = ok & torch.isfinite(corners).all(2).all(1)
    return ok, torch.where(ok[:, None, None], corners, torch.zeros_like(corners))


def _finite_box(vertices):
    """float32 [6] = (lo, hi) of the finite coordinates, per axis, on the vertices' device; zeros for an axis without any."""
    if vertices.shape[0] == 0:
        return torch.zeros([6], dtype=torch.float32, device=vertices.device)
    fin = torch.isfinite(vertices)
    lo = torch.where(fin, vertices, torch.full_like(vertices, math.inf)).amin(0)
    hi = torch.where(fin, vertices, torch.full_like(vertices, -math.inf)).amax(0)
    none = lo > hi
    return torch.cat([torch.where(none, torch.zeros_like(lo), lo), torch.where(none, torch.zeros_like(hi), hi)]).contiguous()


def _dot(u, v):
    s = u[0] * v[0]
    s = s + u[1] * v[1]
    s = s + u[2] * v[2]
    return s


def _sub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


# ---- surface samples --------------------------------------------------------------------------------------------------------
class Samples(NamedTuple):
    """``surface_samples``' result."""
    points: torch.Tensor           # float32 [N, 3]
    face: torch.Tensor             # int64 [N]: the face every point lies on
    capped: torch.Tensor           # int64 scalar on the points' device: the faces that wanted more than k_max subdivisions


def _sample_counts_cpu(vertices, faces32, s2, k_max):
    ok, corners = _corners(vertices, faces32)
    a, b, c = (corners[:, j].unbind(1) for j in range(3))
    sq = lambda u, v: _dot(_sub(v, u), _sub(v, u))                        # noqa: E731
    l2 = torch.maximum(torch.maximum(sq(a, b), sq(b, c)), sq(c, a))
    reaches = lambda k: (k * k).double() * s2 >= l2                        # noqa: E731
    top = torch.full_like(ok, k_max, dtype=torch.int64)
    over = ~reaches(top)
    lo, hi = torch.ones_like(top), top
    for _ in range(k_max.bit_length() + 1):                                # bisection on the monotone predicate
        mid = lo + torch.div(hi - lo, 2, rounding_mode='floor')
        live, r = lo < hi, reaches(mid)
        hi = torch.where(live & r, mid, hi)
        lo = torch.where(live & ~r, mid + 1, lo)
    k = torch.where(over, top, lo)
    return torch.where(ok, k, torch.zeros_like(k)).to(torch.int32), (ok & over).to(torch.uint8)


def _numerators(k):
    """int64 [k^2, 2]: (n0, n1) of the k^2 sub-triangles in the header's order."""
    i, j = torch.meshgrid(torch.arange(k), torch.arange(k), indexing='ij')
    up = (i + j <= k - 1).nonzero()                                        # row-major: i outer, j inner
    down = (i + j <= k - 2).nonzero()
    return torch.cat([3 * up + 1, 3 * down + 2])


def _sample_points_cpu(vertices, faces32, k, offsets, n):
    counts = k.long() ** 2
    f = torch.repeat_interleave(torch.arange(k.shape[0]), counts)
    r, kk = torch.arange(n) - offsets[f], k.long()[f]
    num = torch.zeros([n, 2], dtype=torch.int64)
    for kv in torch.unique(kk).tolist():
        sel = kk == kv
        num[sel] = _numerators(kv)[r[sel]]
    _, corners = _corners(vertices, faces32)
    corners = corners[f]
    n0, n1 = num[:, 0], num[:, 1]
    n2 = 3 * kk - n0 - n1
    s = n0.double()[:, None] * corners[:, 0]
    s = s + n1.double()[:, None] * corners[:, 1]
    s = s + n2.double()[:, None] * corners[:, 2]
    return (s / (3 * kk).double()[:, None]).float(), f.to(torch.int32)


def surface_samples(vertices, faces, spacing, k_max=64):
    """``Samples(points float32 [N, 3], face int64 [N], capped)``: every valid face f is cut into k_f^2 congruent sub-triangles and gives
    their centroids, in a fixed order (include/p3d_hip.h, "mesh distances"), k_f being the smallest integer in [1, k_max] with
    k_f * spacing >= the face's longest edge, decided on squared lengths in fp64 without a square root; a face that would need more
    gets k_max and is counted in ``capped`` (an int64 scalar on the device: no host copy until it is read).  A face with an index
    outside [0, V) or a non-finite corner gives nothing.  Device tensors run two launches with an int64 cumsum between them and copy
    the total to the host, which sizes the output; CPU tensors run the formulation, and the bytes are the same."""
    spacing, k_max = float(spacing), int(k_max)
    if not (spacing > 0.0 and math.isfinite(spacing)):
        raise ValueError(f'surface_samples: spacing must be positive and finite, got {spacing}')
    s2 = spacing * spacing
    if not (s2 > 0.0 and math.isfinite(s2)):
        raise ValueError(f'surface_samples: spacing^2 = {s2} is not a positive finite double')
    if not 1 <= k_max <= K_MAX_CAP:
        raise ValueError(f'surface_samples: k_max must be in [1, {K_MAX_CAP}], got {k_max}')
    vertices, faces32 = _mesh('surface_samples', vertices, faces)
    nv, nf, dev = vertices.shape[0], faces32.shape[0], vertices.device
    if nf == 0:
        return Samples(torch.empty([0, 3], dtype=torch.float32, device=dev), torch.empty([0], dtype=torch.int64, device=dev),
                       torch.zeros([], dtype=torch.int64, device=dev))
    if not vertices.is_cuda:
        k, capped = _sample_counts_cpu(vertices, faces32, s2, k_max)
    else:
        k, capped = torch.empty([nf], dtype=torch.int32, device=dev), torch.empty([nf], dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().p3d_mesh_sample_counts(_lib.ptr(vertices), nv, _lib.ptr(faces32), nf, s2, k_max, _lib.ptr(k), _lib.ptr(capped),
                                                    _lib.stream_of(vertices)), 'mesh_sample_counts')
    offsets = torch.zeros([nf + 1], dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(k.long() ** 2, 0)
    n = int(offsets[-1])                                                   # the one device-to-host copy: sizes the output
    if n >= 2 ** 31 - 1:
        raise ValueError(f'surface_samples: spacing {spacing} gives {n} points, beyond 2^31 - 2; use a larger spacing')
    n_capped = capped.sum(dtype=torch.int64)
    if not vertices.is_cuda:
        points, face = _sample_points_cpu(vertices, faces32, k, offsets, n)
    else:
        points, face = torch.empty([n, 3], dtype=torch.float32, device=dev), torch.empty([n], dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().p3d_mesh_sample_points(_lib.ptr(vertices), nv, _lib.ptr(faces32), nf, _lib.ptr(k), _lib.ptr(offsets), n,
                                                    _lib.ptr(points), _lib.ptr(face), _lib.stream_of(vertices)), 'mesh_sample_points')
    return Samples(points, face.long(), n_capped)


# ---- closest triangle -------------------------------------------------------------------------------------------------------
class Closest(NamedTuple):
    """``closest``'s result."""
    d2: torch.Tensor               # float64 [N]: the squared distance to the nearest valid face, +inf without one
    face: torch.Tensor             # int64 [N]: the smallest id of a face at that distance, -1 without one


class Bvh(NamedTuple):
    """``build_bvh``'s result: the hierarchy over one mesh's faces, on that mesh's device (include/p3d_hip.h, "mesh distances")."""
    tris: torch.Tensor             # float32 [n_leaves * LEAF, 12]: the corners in sorted order, the face id in the first w
    nodes: torch.Tensor            # float32 [2 * n_pad - 1, 8]: the boxes in heap order
    box: torch.Tensor              # float32 [6]: (lo, hi) of the mesh's finite vertices (the frame of the Morton keys)
    n_faces: int
    n_pad: int


def _seg_d2(p, a, b):
    e, r = _sub(b, a), _sub(p, a)
    den, num = _dot(e, e), _dot(r, e)
    pos = den > 0
    t = torch.where(pos, num / torch.where(pos, den, torch.ones_like(den)), torch.zeros_like(den))
    t = t.clamp(0.0, 1.0)
    q = (r[0] - t * e[0], r[1] - t * e[1], r[2] - t * e[2])
    return _dot(q, q)


def _box_d2(p, lo, hi):
    g = tuple(torch.maximum(torch.maximum(lo[k] - p[k], p[k] - hi[k]), torch.zeros_like(p[k])) for k in range(3))
    return _dot(g, g)


def tri_d2(p, a, b, c):
    """include/p3d_hip.h's tri_d2 on broadcastable float64 operands, each a tuple (x, y, z) of tensors: the squared distance
    from p to the closed triangle a b c, one torch operation per rounding.  Total for finite inputs; never a NaN."""
    s = torch.minimum(torch.minimum(_seg_d2(p, a, b), _seg_d2(p, b, c)), _seg_d2(p, c, a))
    e1, e2 = _sub(b, a), _sub(c, a)
    n = _cross(e1, e2)
    nn = _dot(n, n)
    ra, rb, rc = _sub(p, a), _sub(p, b), _sub(p, c)
    wc = _dot(_cross(e1, ra), n)
    wa = _dot(_cross(_sub(c, b), rb), n)
    wb = _dot(_cross(_sub(a, c), rc), n)
    h = _dot(ra, n)
    inside = (nn > 0) & (wa >= 0) & (wb >= 0) & (wc >= 0)
    plane = torch.where(inside, (h * h) / torch.where(inside, nn, torch.ones_like(nn)), s)
    m = torch.minimum(s, plane)
    lo = tuple(torch.minimum(torch.minimum(a[k], b[k]), c[k]) for k in range(3))
    hi = tuple(torch.maximum(torch.maximum(a[k], b[k]), c[k]) for k in range(3))
    return torch.maximum(m, _box_d2(p, lo, hi))


def _closest_cpu(points, vertices, faces32, pairs=1 << 20, face_chunk=4096):
    n = points.shape[0]
    d2 = torch.full([n], math.inf, dtype=torch.float64)
    face = torch.full([n], -1, dtype=torch.int64)
    ok, corners = _corners(vertices, faces32)
    ids = ok.nonzero()[:, 0]                                               # ascending: a later chunk never wins a tie
    live = torch.isfinite(points).all(1).nonzero()[:, 0]
    if not len(ids) or not len(live):
        return Closest(d2, face)
    corners, p64 = corners[ids], points.double()[live]
    step = max(1, pairs // min(face_chunk, len(ids)))
    for p0 in range(0, len(live), step):
        p = tuple(x[:, None] for x in p64[p0:p0 + step].unbind(1))
        best = torch.full([p[0].shape[0]], math.inf, dtype=torch.float64)
        best_id = torch.full([p[0].shape[0]], -1, dtype=torch.int64)
        for f0 in range(0, len(ids), face_chunk):
            tri = corners[f0:f0 + face_chunk]
            a, b, c = (tuple(x[None, :] for x in tri[:, j].unbind(1)) for j in range(3))
            d = tri_d2(p, a, b, c)                                          # [points, faces]
            low = d.min(1).values
            first = torch.where(d == low[:, None], ids[f0:f0 + face_chunk][None, :], torch.iinfo(torch.int64).max).min(1).values
            better = low < best
            best, best_id = torch.where(better, low, best), torch.where(better, first, best_id)
        d2[live[p0:p0 + step]], face[live[p0:p0 + step]] = best, best_id
    return Closest(d2, face)


def build_bvh(vertices, faces):
    """The bounding-volume hierarchy ``closest`` walks for device tensors, reusable across queries of one mesh: a 63-bit Morton key per
    face, a stable sort, leaves of ``LEAF`` consecutive sorted faces and an implicit complete binary tree of fp32 boxes above them,
    built one level per launch, bottom up (include/p3d_hip.h, "mesh distances").  No host copy.  A uniform grid was considered and rejected: a
    query far from the target walks O(r^3) empty cells, and two meshes that are compared need not overlap."""
    vertices, faces32 = _mesh('build_bvh', vertices, faces)
    if not vertices.is_cuda:
        raise ValueError('build_bvh: CPU tensors run the all-pairs definition and take no hierarchy')
    nv, nf, dev = vertices.shape[0], faces32.shape[0], vertices.device
    n_leaves = -(-nf // LEAF)
    n_pad = 1 << max(n_leaves - 1, 0).bit_length()
    if n_pad.bit_length() > MAX_DEPTH:
        raise ValueError(f'build_bvh: {nf} faces need a tree deeper than {MAX_DEPTH}')
    box = _finite_box(vertices)
    key = torch.empty([nf], dtype=torch.int64, device=dev)
    lib = _lib.lib()
    _lib.check(lib.p3d_mesh_bvh_keys(_lib.ptr(vertices), nv, _lib.ptr(faces32), nf, _lib.ptr(box), _lib.ptr(key), _lib.stream_of(vertices)),
               'mesh_bvh_keys')
    order = torch.sort(key, stable=True).indices.to(torch.int32)
    tris = torch.empty([n_leaves * LEAF, 12], dtype=torch.float32, device=dev)
    nodes = torch.empty([2 * n_pad - 1, 8], dtype=torch.float32, device=dev)
    _lib.check(lib.p3d_mesh_bvh_build(_lib.ptr(vertices), nv, _lib.ptr(faces32), nf, _lib.ptr(order), n_pad, _lib.ptr(tris), _lib.ptr(nodes),
                                      _lib.stream_of(vertices)), 'mesh_bvh_build')
    return Bvh(tris, nodes, box, nf, n_pad)


def _closest_device(points, bvh, sort_queries):
    n, dev = points.shape[0], points.device
    lib = _lib.lib()
    order = None
    if n and (n >= SORT_QUERIES_FROM if sort_queries is None else sort_queries) and n < 2 ** 31 - 1:
        key = torch.empty([n], dtype=torch.int64, device=dev)              # neighbours in the wave walk the same nodes
        _lib.check(lib.p3d_mesh_bvh_keys(_lib.ptr(points), n, None, n, _lib.ptr(bvh.box), _lib.ptr(key), _lib.stream_of(points)), 'mesh_bvh_keys')
        order = torch.sort(key, stable=True).indices
        points = points[order].contiguous()
    d2 = torch.empty([n], dtype=torch.float64, device=dev)
    face = torch.empty([n], dtype=torch.int64, device=dev)
    status = torch.zeros([1], dtype=torch.int32, device=dev)
    _lib.check(lib.p3d_mesh_closest(_lib.ptr(points), n, _lib.ptr(bvh.tris), _lib.ptr(bvh.nodes), bvh.n_faces, bvh.n_pad, _lib.ptr(d2), _lib.ptr(face),
                                    _lib.ptr(status), _lib.stream_of(points)), 'mesh_closest')
    if n and int(status):                                                  # one device-to-host copy: the walk's own bound
        raise RuntimeError(f'mesh_closest: libp3d_hip error {_lib.P3D_ERR_LAUNCH}: a tree walk passed its iteration bound (the hierarchy is not one build_bvh made)')
    if order is None:
        return Closest(d2, face)
    out_d2, out_face = torch.empty_like(d2), torch.empty_like(face)
    out_d2[order], out_face[order] = d2, face
    return Closest(out_d2, out_face)


def closest(points, vertices, faces, bvh=None, sort_queries=None):
    """``Closest(d2 float64 [N], face int64 [N])``: for every point the minimum over the mesh's valid faces of ``tri_d2`` (the squared
    distance to the closed triangle, fp64 from the fp32 inputs, stated operation by operation in include/p3d_hip.h, "mesh distances") and the
    smallest face id that attains it.  A face with an index outside [0, V) or a non-finite corner has distance +inf; a non-finite
    point gets (+inf, -1), and so does every point when no face is valid.  The points' device picks the path and the mesh is moved
    there.  CPU tensors run THE DEFINITION: all N T pairs in chunks — meant for tests and small inputs, not for the 10^6 x 10^6 pairs
    of a 512^3 mesh.  Device tensors walk ``bvh`` (``build_bvh(vertices, faces)``, built here when not given; pass it to query one mesh
    more than once) and return the same bits, whatever the order of points or faces.  ``sort_queries`` sorts the points by Morton key
    before the launch and unsorts after (None: from ``SORT_QUERIES_FROM`` points on); only the time depends on it.  One
    device-to-host copy, of the walk's status word."""
    points = _points('closest', points)
    if bvh is not None and points.is_cuda:
        if bvh.nodes.device != points.device or (faces is not None and bvh.n_faces != faces.shape[0]):
            raise ValueError('closest: bvh belongs to another mesh or device')
        return _closest_device(points, bvh, sort_queries)
    vertices, faces32 = _mesh('closest', vertices.to(points.device), faces)
    if not points.is_cuda:
        return _closest_cpu(points, vertices, faces32)
    return _closest_device(points, build_bvh(vertices, faces32), sort_queries)


# ---- metrics ----------------------------------------------------------------------------------------------------------------
class Direction(NamedTuple):
    """The distances from the samples of one mesh to another mesh.  ``mean``, ``rms`` and ``max`` are float64 scalars on the
    distances' device and ``within`` is int64 [K]: nothing is copied to the host until a field is read.  mean and rms are fp64 torch
    reductions, floats that differ between devices by the order of an fp64 sum (about 1e-12 relative); ``within`` and ``max`` do not."""
    n: int
    mean: torch.Tensor
    rms: torch.Tensor
    max: torch.Tensor              # the sampled one-sided Hausdorff distance
    within: torch.Tensor           # int64 [K]: the samples with distance <= thresholds[j]


class GeometryAgreement(NamedTuple):
    """``distance_stats``' and ``compare``'s result: ``forward`` from A's samples to B, ``backward`` from B's to A (None for one
    direction).  The two-direction figures below need both."""
    thresholds: tuple
    forward: Direction
    backward: Optional[Direction] = None

    @property
    def hausdorff(self):
        """The sampled symmetric Hausdorff distance: the larger of the two one-sided maxima (one direction: its maximum)."""
        return self.forward.max if self.backward is None else torch.maximum(self.forward.max, self.backward.max)

    @property
    def chamfer(self):
        """The sum of the two mean distances."""
        return self.forward.mean + self.backward.mean

    @property
    def precision(self):
        """float64 [K]: the share of A's samples within each threshold of B."""
        return self.forward.within.double() / max(self.forward.n, 1)

    @property
    def recall(self):
        """float64 [K]: the share of B's samples within each threshold of A."""
        return self.backward.within.double() / max(self.backward.n, 1)

    @property
    def fscore(self):
        """float64 [K]: 2 P R / (P + R), 0 where both are 0."""
        p, r = self.precision, self.recall
        s = p + r
        return torch.where(s > 0, 2.0 * p * r / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(s))


def _thresholds(what, thresholds):
    thresholds = tuple(float(t) for t in thresholds)
    if any(not (t >= 0.0 and math.isfinite(t)) for t in thresholds) or any(a >= b for a, b in zip(thresholds, thresholds[1:])):
        raise ValueError(f'{what}: thresholds must be finite, non-negative and ascending, got {thresholds}')
    return thresholds


def _direction(d2, thresholds):
    d2 = torch.as_tensor(d2).detach()
    if d2.dtype != torch.float64 or d2.ndim != 1:
        raise ValueError(f'distance_stats: d2 must be float64 [N], got {d2.dtype} {tuple(d2.shape)}')
    squared = torch.tensor([t * t for t in thresholds], dtype=torch.float64).to(d2.device)
    bucket = torch.searchsorted(squared, d2)                               # the first threshold with d2 <= t^2: an integer, the same everywhere
    within = (bucket[None, :] <= torch.arange(len(thresholds), device=d2.device)[:, None]).sum(1)      # (no bincount: on a device it copies its size to the host)
    if d2.shape[0] == 0:
        zero = torch.zeros([], dtype=torch.float64, device=d2.device)
        return Direction(0, zero, zero, zero, within)
    return Direction(d2.shape[0], d2.sqrt().mean(), d2.mean().sqrt(), d2.max().sqrt(), within)


def distance_stats(d2, thresholds, backward=None):
    """``GeometryAgreement`` of squared distances float64 [N] as ``closest`` gives them (and, with ``backward``, of the other
    direction's): per direction the number of samples, the mean distance, the RMS, the maximum and the int64 counts of samples within
    each of the ascending ``thresholds`` (distances; decided as d2 <= t^2 by an integer ``searchsorted``, so the counts are exact and
    equal on every device).  A sample without any face (d2 = +inf) is within nothing and makes mean, rms and max infinite.  No host
    synchronisation."""
    thresholds = _thresholds('distance_stats', thresholds)
    return GeometryAgreement(thresholds, _direction(d2, thresholds), None if backward is None else _direction(backward, thresholds))


def diagonal(vertices):
    """The length of the diagonal of the bounding box of the finite vertices, a Python float (on a device: one device-to-host copy)."""
    lo, hi = _finite_box(mesh._vertices32('diagonal', vertices)).double().cpu().view(2, 3).tolist()
    return math.sqrt(sum((h - l) * (h - l) for l, h in zip(lo, hi)))


def compare(va, fa, vb, fb, spacing=None, thresholds=None, k_max=64):
    """``GeometryAgreement`` of mesh A (va, fa) and mesh B (vb, fb), both directions: ``surface_samples`` of each at ``spacing`` (default:
    the diagonal of A's bounding box over 512) against ``closest`` on the other.  ``thresholds`` default to 0.25 %, 0.5 % and 1 % of
    that diagonal.  A's device picks the path.  The counts are equal on both paths, d2 bit for bit; mean and rms are within the 1e-12
    of an fp64 sum's order.  Host copies: the diagonal, the two sample totals and the two status words."""
    va, fa32 = _mesh('compare', va, fa)
    vb, fb32 = _mesh('compare', vb.to(va.device), fb)
    diag = diagonal(va) if spacing is None or thresholds is None else None
    spacing = diag / 512 if spacing is None else float(spacing)
    thresholds = tuple(diag * t for t in (0.0025, 0.005, 0.01)) if thresholds is None else _thresholds('compare', thresholds)
    sa, sb = surface_samples(va, fa32, spacing, k_max), surface_samples(vb, fb32, spacing, k_max)
    return distance_stats(closest(sa.points, vb, fb32).d2, thresholds, closest(sb.points, va, fa32).d2)


# ---- colours ----------------------------------------------------------------------------------------------------------------
def _palette(palette):
    j = torch.arange(256, dtype=torch.int64)
    if palette == 'heat':                                                  # black, red, yellow, white
        table = torch.stack([(3 * j).clamp(0, 255), (3 * j - 255).clamp(0, 255), (3 * j - 510).clamp(0, 255)], 1)
    elif palette == 'grey':
        table = torch.stack([j, j, j], 1)
    else:
        table = None if isinstance(palette, str) else torch.as_tensor(palette)
        if table is None or tuple(table.shape) != (256, 3):
            raise ValueError("distance_colors: palette must be 'heat', 'grey' or a uint8 [256, 3] table")
    return table.to(torch.uint8)


def distance_colors(d2, scale, palette='heat'):
    """uint8 [N, 3] colours of squared distances float64 [N]: row j of a 256-entry integer table, j being the number of edges
    (scale * i / 255)^2, i = 1 .. 255, that are <= d2 (a ``searchsorted``): 0 below scale / 255, 255 from ``scale`` on and for +inf.
    Feed it ``closest(vertices_b, va, fa).d2`` for the error heat map of mesh B against A as vertex colours."""
    scale = float(scale)
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError(f'distance_colors: scale must be positive and finite, got {scale}')
    d2 = torch.as_tensor(d2).detach().double()
    edges = torch.tensor([(scale * i / 255) * (scale * i / 255) for i in range(1, 256)], dtype=torch.float64).to(d2.device)
    return _palette(palette).to(d2.device)[torch.searchsorted(edges, d2, right=True)]


# ---- what an edit did to the shape ----------------------------------------------------------------------------------------------
class ChangeMap(NamedTuple):
    """``change_map``'s result."""
    vertices: torch.Tensor         # the "after" mesh
    faces: torch.Tensor
    d2: torch.Tensor               # float64 [V]: every "after" vertex's squared distance to the "before" mesh
    agreement: GeometryAgreement   # A = after, B = before
    colors: torch.Tensor           # uint8 [V, 3]: ``distance_colors(d2, scale)``
    frames: Optional[torch.Tensor]      # uint8 [n_frames, image_size, image_size, 3] in those colours, or None


@torch.no_grad()
def change_map(G, ws_before, ws_after, resolution=128, threshold=50., n_frames=0, image_size=512, scale=None, spacing=None,
               thresholds=None, palette='heat', **synthesis_kwargs):
    """Where in 3D the shape of ``ws_after`` differs from that of ``ws_before`` (two latents of G, e.g. of an edit session before and
    after a stroke): both meshes through ``shape.extract_geometry``, the per-vertex distance of the "after" mesh to the "before"
    mesh, their ``compare`` and, for n_frames > 0, the script's turntable of the "after" mesh in heat colours (``scale``: the distance
    that maps to the table's end, default 1 % of the "after" mesh's diagonal)."""
    vb, fb = shape.extract_geometry(G, ws_before, resolution, threshold, **synthesis_kwargs)
    va, fa = shape.extract_geometry(G, ws_after, resolution, threshold, **synthesis_kwargs)
    d2 = closest(va, vb, fb).d2
    agreement = compare(va, fa, vb, fb, spacing, thresholds)
    scale = 0.01 * diagonal(va) if scale is None else float(scale)
    colors = distance_colors(d2, scale, palette) if len(va) else torch.empty([0, 3], dtype=torch.uint8, device=va.device)
    frames = None
    if n_frames > 0:
        poses, camera = mesh.script_turntable(G, n_frames)
        frames = mesh.render(va, fa, poses, camera, image_size, colors=colors)
    return ChangeMap(va, fa, d2, agreement, colors, frames)
