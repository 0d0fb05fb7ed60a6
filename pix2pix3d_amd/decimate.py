"""Quadric-error decimation: what a trimesh or MeshLab user runs on an extracted mesh (``simplify_quadric_decimation``), as ROUNDS of edge collapses.

``mesh.simplify`` clusters vertices on a grid: fast, but it rounds every ridge to the cell, pinches necks, and has no face target.  Here every vertex
carries the quadric of its input faces' planes (Garland & Heckbert 1997), an edge is rated by the quadric error of its best merged position, and every
round collapses at once a set of cheap edges no two of which touch each other's 1-rings — so that the result is a pure function of the input, whatever
order the hardware takes the edges in.  Only interior edges of a 2-manifold neighbourhood collapse (boundary and ``pinned`` vertices, fins and edges
whose link condition fails are never touched), and a collapse that would turn a face over or into a spike is refused, so a closed manifold stays a
closed manifold.  The rules are csrc/mesh/p3d_mesh.h's; DESIGN.md section 2.1aa has the measurements.

    decimate(vertices, faces, target_faces, fraction, max_rounds, pinned)   -> Decimation
    decimate_to(vertices, faces, tolerance, spacing)                        -> (vertices', faces', target_faces or None, agreement)

CPU tensors run the torch formulation below, which is the definition; device tensors run the kernels of csrc/mesh/mesh_decimate.hip through
``mesh_lib()`` (libp3d_mesh.so, a kernel library of its own beside libp3d_hip.so) with the same bytes.  The sorts and scans between the kernels
(``mesh.adjacency``, the vertex -> face list, the ranks) are torch on the tensors' device for both."""
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, mesh

_side = _lib.SideLibrary('mesh')                     # libp3d_mesh.so: loaded on the first call, device-guarded; launch_count() is its own counter
MESH_LIB_PATH, HEADER = _side.path, _side.header
mesh_lib, launch_count, _check = _side.lib, _side.launch_count, _side.check
NO_RANK = HEADER.constants['P3D_MESH_NO_RANK']
QUADRIC = HEADER.constants['P3D_MESH_QUADRIC_DOUBLES']
MAX_COUNT = HEADER.constants['P3D_MESH_DECIMATE_MAX']
LAUNCHES_PER_ROUND = 6         # p3d_mesh_edge_costs 1, p3d_mesh_edge_select 3, p3d_mesh_collapse 2 (and p3d_mesh_quadrics once a call)
DECIMATE_RUNGS = 40            # decimate_to's ladder of targets: T / 2^(i / 2), i = 1 .. 40, as long as they stay at 4 faces or more


class Decimation(NamedTuple):
    """``decimate``'s result."""
    vertices: torch.Tensor         # float32 [V', 3]: the vertices the faces use, in input order
    faces: torch.Tensor            # int64 [T', 3], in input order
    vertex_map: torch.Tensor       # int64 [V]: the output index of the vertex v was merged into (its own if it survived), -1 where no output face uses it
    rounds: int                    # the rounds that collapsed something
    reached: bool                  # T' <= target_faces


# ---- fp64 vectors as tuples of tensors: one torch operation per rounding ----------------------------------------------------------------------
def _xyz(v64, idx):
    p = v64[idx]
    return p[:, 0], p[:, 1], p[:, 2]


def _sub(u, v):
    return u[0] - v[0], u[1] - v[1], u[2] - v[2]


def _dot(u, v):
    s = u[0] * v[0]
    s = s + u[1] * v[1]
    s = s + u[2] * v[2]
    return s


def _cross(u, v):
    return u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]


def _normal(a, b, c):
    return _cross(_sub(b, a), _sub(c, a))


def _sqrt(x):
    """The correctly rounded fp64 square root, which the kernels and the rules mean.  torch.sqrt on CPU doubles goes through a vector maths library that
    is within one unit of the last place only (about one value in a hundred differs, and which ones depends on the processor); numpy's is the
    hardware's instruction."""
    return torch.from_numpy(np.sqrt(x.numpy())) if x.device.type == 'cpu' else torch.sqrt(x)


# ---- lists --------------------------------------------------------------------------------------------------------------------------
def vertex_faces(faces, n_vertices):
    """The vertex -> face list of p3d_mesh.h: (offsets int64 [V + 1], faces int32 [3 T]), a stable sort of the corners by their vertex."""
    corner, order = torch.sort(faces.reshape(-1).long(), stable=True)
    offsets = torch.searchsorted(corner, torch.arange(n_vertices + 1, device=faces.device))
    return offsets, torch.div(order, 3, rounding_mode='floor').to(torch.int32)


def _expand(offsets, owners):
    """Every entry of the lists of ``owners`` (vertex ids [N]): (row int64 [M] into owners, entry int64 [M] into the list), rows ascending and a
    row's entries in list order."""
    start = offsets[owners]
    counts = offsets[owners + 1] - start
    row = torch.repeat_interleave(torch.arange(len(owners), device=owners.device), counts)
    first = torch.cumsum(counts, 0) - counts
    return row, start[row] + (torch.arange(len(row), device=owners.device) - first[row])


class Round(NamedTuple):
    """The lists of a round, from the current faces (torch on the faces' device; the header's lists)."""
    adj: mesh.Adjacency
    entry_edge: torch.Tensor       # int32 [n_entries]: the edge id of every adjacency entry
    edges: torch.Tensor            # int32 [E, 2]: (a, b), a < b, ascending a * V + b
    vf_offsets: torch.Tensor       # int64 [V + 1]
    vf_faces: torch.Tensor         # int32 [3 T]


def round_lists(faces32, n_vertices):
    faces = faces32.long()
    adj = mesh.adjacency(faces, n_vertices)
    n_entries, dev = adj.neighbours.shape[0], faces.device
    source = torch.repeat_interleave(torch.arange(n_vertices, device=dev), adj.offsets[1:] - adj.offsets[:-1], output_size=n_entries)
    nb = adj.neighbours.long()
    upper = nb > source
    eid = torch.cumsum(upper, 0) - 1
    twin = torch.searchsorted(source * n_vertices + nb, nb * n_vertices + source)      # the entry (w, v) of the entry (v, w): the keys are sorted
    entry_edge = torch.where(upper, eid, eid[twin.clamp(max=max(n_entries - 1, 0))]).to(torch.int32)
    edges = torch.stack([source[upper], nb[upper]], 1).to(torch.int32).contiguous()
    return Round(adj, entry_edge, edges, *vertex_faces(faces, n_vertices))


# ---- rule 1: quadrics ---------------------------------------------------------------------------------------------------------------------
def _quadrics_torch(vertices, faces32, vf_offsets, vf_faces):
    v64, faces = vertices.double(), faces32.long()
    a, b, c = (_xyz(v64, faces[:, k]) for k in range(3))
    n = _normal(a, b, c)
    nn = _dot(n, n)
    live = nn > 0
    length = _sqrt(torch.where(live, nn, torch.ones_like(nn)))
    h = (n[0] / length, n[1] / length, n[2] / length)
    p = h + (-_dot(h, a),)
    w = length * 0.5
    k_face = torch.stack([w * (p[r] * p[c2]) for r in range(4) for c2 in range(r, 4)], 1)
    k_face = torch.where(live[:, None], k_face, torch.zeros_like(k_face))
    counts = vf_offsets[1:] - vf_offsets[:-1]
    acc = torch.zeros([vertices.shape[0], QUADRIC], dtype=torch.float64, device=vertices.device)
    live_v = (counts > 0).nonzero()[:, 0]
    j = 0
    while len(live_v):                                                       # one list position of every vertex per pass: list order
        acc[live_v] = acc[live_v] + k_face[vf_faces[vf_offsets[live_v] + j].long()]
        j += 1
        live_v = live_v[counts[live_v] > j]
    return acc


def quadrics(vertices, faces32, vf_offsets, vf_faces):
    """Rule 1: float64 [V, 10]."""
    if not vertices.is_cuda:
        return _quadrics_torch(vertices, faces32, vf_offsets, vf_faces)
    q = torch.empty([vertices.shape[0], QUADRIC], dtype=torch.float64, device=vertices.device)
    _check(mesh_lib().p3d_mesh_quadrics(_lib.ptr(vertices), vertices.shape[0], _lib.ptr(faces32), faces32.shape[0], _lib.ptr(vf_offsets),
                                                           _lib.ptr(vf_faces), _lib.ptr(q), _lib.stream_of(q)), 'mesh_quadrics')
    return q


# ---- rules 2 and 3: validity, target point, cost ------------------------------------------------------------------------------------------------
def _cost(q, x):
    r0 = q[0] * x[0]; r0 = r0 + q[1] * x[1]; r0 = r0 + q[2] * x[2]; r0 = r0 + q[3]
    r1 = q[1] * x[0]; r1 = r1 + q[4] * x[1]; r1 = r1 + q[5] * x[2]; r1 = r1 + q[6]
    r2 = q[2] * x[0]; r2 = r2 + q[5] * x[1]; r2 = r2 + q[7] * x[2]; r2 = r2 + q[8]
    r3 = q[3] * x[0]; r3 = r3 + q[6] * x[1]; r3 = r3 + q[8] * x[2]; r3 = r3 + q[9]
    c = x[0] * r0; c = c + x[1] * r1; c = c + x[2] * r2; c = c + r3
    return torch.where(c > 0, c, torch.zeros_like(c))


def _take(take, new, old):
    return tuple(torch.where(take, n, o) for n, o in zip(new, old))


def _edge_costs_torch(vertices, quads, faces32, lists, fixed):
    v64, faces, dev = vertices.double(), faces32.long(), vertices.device
    nv, adj = vertices.shape[0], lists.adj
    ea, eb = lists.edges[:, 0].long(), lists.edges[:, 1].long()
    ne = len(ea)
    ok = (fixed[ea] == 0) & (fixed[eb] == 0)
    # the faces that use the edge and their third corners
    row, entry = _expand(lists.vf_offsets, ea)
    x = faces[lists.vf_faces[entry].long()]
    ra, rb = ea[row], eb[row]
    uses_b = (x == rb[:, None]).any(1)
    end0, end1 = (x[:, 0] == ra) | (x[:, 0] == rb), (x[:, 1] == ra) | (x[:, 1] == rb)
    third = torch.where(~end0, x[:, 0], torch.where(~end1, x[:, 1], x[:, 2]))
    r, third = row[uses_b], third[uses_b]
    uses = torch.zeros([ne], dtype=torch.int64, device=dev).index_add_(0, r, torch.ones_like(r))
    nth = torch.arange(len(r), device=dev) - (torch.cumsum(uses, 0) - uses)[r]
    t0, t1 = torch.full([ne], -1, dtype=torch.int64, device=dev), torch.full([ne], -1, dtype=torch.int64, device=dev)
    t0[r[nth == 0]] = third[nth == 0]
    t1[r[nth == 1]] = third[nth == 1]
    ok &= (uses == 2) & (t0 != t1)
    # the link condition
    counts = adj.offsets[1:] - adj.offsets[:-1]
    n_entries = adj.neighbours.shape[0]
    key = torch.repeat_interleave(torch.arange(nv, device=dev), counts, output_size=n_entries) * nv + adj.neighbours.long()
    row, entry = _expand(adj.offsets, ea)
    u = adj.neighbours[entry].long()
    probe = eb[row] * nv + u
    common = key[torch.searchsorted(key, probe).clamp(max=max(n_entries - 1, 0))] == probe
    r, u = row[common], u[common]
    n_common = torch.zeros([ne], dtype=torch.int64, device=dev).index_add_(0, r, torch.ones_like(r))
    lo = torch.full([ne], nv, dtype=torch.int64, device=dev).scatter_reduce_(0, r, u, 'amin')
    hi = torch.full([ne], -1, dtype=torch.int64, device=dev).scatter_reduce_(0, r, u, 'amax')
    min_degree = torch.full([ne], 1 << 40, dtype=torch.int64, device=dev).scatter_reduce_(0, r, counts[u], 'amin')
    ok &= (n_common == 2) & (lo == torch.minimum(t0, t1)) & (hi == torch.maximum(t0, t1)) & (min_degree >= 4) & (counts[ea] + counts[eb] - 4 >= 4)
    # the target point and its cost
    q = (quads[ea] + quads[eb]).unbind(1)
    pa, pb = _xyz(v64, ea), _xyz(v64, eb)
    mid = tuple((pa[k] + pb[k]) * 0.5 for k in range(3))
    best, best_cost = pa, _cost(q, pa)
    for cand in (pb, mid):
        c = _cost(q, cand)
        take = c < best_cost
        best, best_cost = _take(take, cand, best), torch.where(take, c, best_cost)
    c00, c01, c02 = q[4] * q[7] - q[5] * q[5], q[2] * q[5] - q[1] * q[7], q[1] * q[5] - q[2] * q[4]
    c11, c12, c22 = q[0] * q[7] - q[2] * q[2], q[1] * q[2] - q[0] * q[5], q[0] * q[4] - q[1] * q[1]
    det = q[0] * c00; det = det + q[1] * c01; det = det + q[2] * c02
    m = torch.stack([q[k].abs() for k in (0, 1, 2, 4, 5, 7)]).max(0).values
    bound = m * m; bound = bound * m; bound = bound * 2.0 ** -20
    solvable = det.abs() > bound
    den = torch.where(solvable, det, torch.ones_like(det))
    r0 = c00 * q[3]; r0 = r0 + c01 * q[6]; r0 = r0 + c02 * q[8]
    r1 = c01 * q[3]; r1 = r1 + c11 * q[6]; r1 = r1 + c12 * q[8]
    r2 = c02 * q[3]; r2 = r2 + c12 * q[6]; r2 = r2 + c22 * q[8]
    s = ((-r0) / den, (-r1) / den, (-r2) / den)
    off, ab = _sub(s, mid), _sub(pb, pa)
    c = _cost(q, s)
    take = solvable & (_dot(off, off) <= _dot(ab, ab) * 4.0) & (c < best_cost)
    best, best_cost = _take(take, s, best), torch.where(take, c, best_cost)
    ok &= best_cost < math.inf
    target = torch.stack(best, 1).float()
    # the flip test, at the fp32 target, over the edges that are still valid
    idx = ok.nonzero()[:, 0]
    flipped = torch.zeros([ne], dtype=torch.bool, device=dev)
    p64 = target.double()
    for v, other in ((ea[idx], eb[idx]), (eb[idx], ea[idx])):
        row, entry = _expand(lists.vf_offsets, v)
        x = faces[lists.vf_faces[entry].long()]
        skip = (x == other[row][:, None]).any(1)
        corners = [_xyz(v64, x[:, k]) for k in range(3)]
        n0 = _normal(*corners)
        nn0 = _dot(n0, n0)
        p = _xyz(p64, idx[row])
        moved = [_take(x[:, k] == v[row], p, corners[k]) for k in range(3)]
        n1 = _normal(*moved)
        nn1, d = _dot(n1, n1), _dot(n0, n1)
        good = skip | ~(nn0 > 0) | ((d > 0) & (d * d >= (nn0 * nn1) * 0.0625))
        flipped[idx[row[~good]]] = True
    ok &= ~flipped
    return (torch.where(ok[:, None], target, torch.zeros_like(target)), torch.where(ok, best_cost, torch.full_like(best_cost, math.inf)),
            ok.to(torch.uint8))


def edge_costs(vertices, quads, faces32, lists, fixed):
    """Rules 2 and 3 for every edge of ``lists``: (target float32 [E, 3], cost float64 [E], valid uint8 [E]); ``fixed`` uint8 [V]."""
    if not vertices.is_cuda:
        return _edge_costs_torch(vertices, quads, faces32, lists, fixed)
    ne, dev, adj = lists.edges.shape[0], vertices.device, lists.adj
    target = torch.empty([ne, 3], dtype=torch.float32, device=dev)
    cost = torch.empty([ne], dtype=torch.float64, device=dev)
    valid = torch.empty([ne], dtype=torch.uint8, device=dev)
    _check(mesh_lib().p3d_mesh_edge_costs(
        _lib.ptr(vertices), _lib.ptr(quads), vertices.shape[0], _lib.ptr(faces32), faces32.shape[0], _lib.ptr(adj.offsets), _lib.ptr(adj.neighbours),
        adj.neighbours.shape[0], _lib.ptr(fixed), _lib.ptr(lists.vf_offsets), _lib.ptr(lists.vf_faces), _lib.ptr(lists.edges), ne, _lib.ptr(target),
        _lib.ptr(cost), _lib.ptr(valid), _lib.stream_of(target)), 'mesh_edge_costs')
    return target, cost, valid


# ---- rules 4 and 5: order, candidates, independent set ---------------------------------------------------------------------------------------------
def mix(x):
    """The 32-bit bijection of rule 4 on an int64 tensor of values below 2^32 (products kept below 2^63)."""
    mask = 0xffffffff

    def times(x, c):
        return ((x & 0xffff) * c + (((x >> 16) * c & 0xffff) << 16)) & mask
    x = x ^ (x >> 16)
    x = times(x, 0x7feb352d)
    x = x ^ (x >> 15)
    x = times(x, 0x846ca68b)
    return x ^ (x >> 16)


def candidate_ranks(cost, valid, n_faces, target_faces, fraction):
    """(perm int64 [E]: the edges by (cost, mix(id)); rank int32 [E]: a candidate's rank, NO_RANK elsewhere; need).  Nothing is copied to the host."""
    ne, dev = cost.shape[0], cost.device
    by_mix = torch.argsort(mix(torch.arange(ne, device=dev)))
    perm = by_mix[torch.sort(cost[by_mix], stable=True).indices]
    need = (n_faces - target_faces + 1) // 2
    k = torch.ceil(valid.sum().double() * fraction).clamp(min=1).clamp(max=need).long()
    tau = cost[perm].index_select(0, (k - 1).reshape(1))
    rank = torch.empty([ne], dtype=torch.int32, device=dev)
    rank[perm] = torch.arange(ne, dtype=torch.int32, device=dev)
    return perm, torch.where((valid != 0) & (cost <= tau), rank, torch.full_like(rank, NO_RANK)), need


def _edge_select_torch(rank, lists, n_vertices):
    adj, dev = lists.adj, rank.device
    n_entries = adj.neighbours.shape[0]
    source = torch.repeat_interleave(torch.arange(n_vertices, device=dev), adj.offsets[1:] - adj.offsets[:-1], output_size=n_entries)
    m1 = torch.full([n_vertices], NO_RANK, dtype=torch.int32, device=dev).scatter_reduce_(0, source, rank[lists.entry_edge.long()], 'amin')
    m2 = m1.clone().scatter_reduce_(0, source, m1[adj.neighbours.long()], 'amin')
    ea, eb = lists.edges[:, 0].long(), lists.edges[:, 1].long()
    return ((rank != NO_RANK) & (rank == m2[ea]) & (rank == m2[eb])).to(torch.uint8)


def edge_select(rank, lists, n_vertices):
    """Rule 5: uint8 [E], the candidates whose rank is the smallest within the 1-rings of both ends."""
    if not rank.is_cuda:
        return _edge_select_torch(rank, lists, n_vertices)
    adj, dev, ne = lists.adj, rank.device, rank.shape[0]
    m1, m2 = torch.empty([n_vertices], dtype=torch.int32, device=dev), torch.empty([n_vertices], dtype=torch.int32, device=dev)
    win = torch.empty([ne], dtype=torch.uint8, device=dev)
    _check(mesh_lib().p3d_mesh_edge_select(_lib.ptr(rank), _lib.ptr(lists.edges), ne, n_vertices, _lib.ptr(adj.offsets),
                                                              _lib.ptr(adj.neighbours), _lib.ptr(lists.entry_edge), adj.neighbours.shape[0], _lib.ptr(m1),
                                                              _lib.ptr(m2), _lib.ptr(win), _lib.stream_of(win)), 'mesh_edge_select')
    return win


def applied_edges(win, perm, need):
    """uint8 [E]: of the winners, the ``need`` lowest ranks."""
    by_rank = win[perm] != 0
    apply = torch.empty_like(win)
    apply[perm] = (by_rank & (torch.cumsum(by_rank, 0) <= need)).to(torch.uint8)
    return apply


# ---- rule 6: collapse -----------------------------------------------------------------------------------------------------------------------
def _collapse_torch(vertices, quads, parent, faces32, edges, apply, target):
    idx = (apply != 0).nonzero()[:, 0]
    a, b = edges[idx, 0].long(), edges[idx, 1].long()
    vertices[a] = target[idx]
    quads[a] = quads[a] + quads[b]
    parent[b] = a.to(torch.int32)
    faces32.copy_(parent[faces32.long()])
    return ((faces32[:, 0] == faces32[:, 1]) | (faces32[:, 1] == faces32[:, 2]) | (faces32[:, 0] == faces32[:, 2])).to(torch.uint8)


def collapse(vertices, quads, parent, faces32, edges, apply, target):
    """Rule 6, IN PLACE on vertices, quads, parent int32 [V] and faces32; returns dead uint8 [T], the faces with two equal corners."""
    if not vertices.is_cuda:
        return _collapse_torch(vertices, quads, parent, faces32, edges, apply, target)
    dead = torch.empty([faces32.shape[0]], dtype=torch.uint8, device=vertices.device)
    _check(mesh_lib().p3d_mesh_collapse(_lib.ptr(vertices), _lib.ptr(quads), _lib.ptr(parent), vertices.shape[0], _lib.ptr(faces32),
                                                           faces32.shape[0], _lib.ptr(edges), _lib.ptr(apply), _lib.ptr(target), edges.shape[0], _lib.ptr(dead),
                                                           _lib.stream_of(dead)), 'mesh_collapse')
    return dead


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def default_max_rounds(n_faces):
    return 16 * math.ceil(math.log2(max(n_faces, 1))) + 64


def decimate(vertices, faces, target_faces, fraction=0.25, max_rounds=None, pinned=None):
    """Quadric-error decimation of the mesh (vertices [V, 3], faces int32 / int64 [T, 3]) towards ``target_faces`` faces: a ``Decimation``.  Every round
    rates every edge, takes the cheapest ``fraction`` of the valid ones (never more than are needed) as candidates, and collapses those whose rank is the
    smallest within the 1-rings of both their ends; it stops at the target (``reached``), when no edge is valid any more, or after ``max_rounds`` rounds
    (default 16 ceil(log2 T) + 64).  A collapse removes two faces, so T' >= target_faces - 1.  ``pinned`` bool [V] vertices, like boundary vertices, neither
    move nor merge.  Only positions are carried: colour the result afterwards.  Operand checks are ``mesh``'s (a bad index or a non-finite vertex is a
    ValueError before any launch); a mesh without vertices or faces comes back as it is, with the identity as its map.  One scalar is copied to the host per
    round (not graph-capturable, like ``mesh.simplify``)."""
    if isinstance(target_faces, bool) or int(target_faces) != target_faces or target_faces < 0:
        raise ValueError(f'decimate: target_faces must be a non-negative integer, got {target_faces!r}')
    target_faces, fraction = int(target_faces), float(fraction)
    if not 0.0 < fraction <= 1.0:
        raise ValueError(f'decimate: fraction must be in (0, 1], got {fraction}')
    vertices = mesh._mesh_vertices('decimate', vertices)
    nv, dev = vertices.shape[0], vertices.device
    faces = mesh._mesh_faces('decimate', faces, nv).to(dev)
    nf = faces.shape[0]
    if max(nv, nf) >= MAX_COUNT:
        raise ValueError(f'decimate: {nv} vertices and {nf} faces, beyond the 2^30 the kernels take')
    max_rounds = default_max_rounds(nf) if max_rounds is None else mesh._iterations('decimate', max_rounds)
    mesh._pinned('decimate', pinned, nv, dev)                                # (checked even when nothing runs)
    if nv == 0 or nf == 0:
        return Decimation(vertices, faces, torch.arange(nv, dtype=torch.int64, device=dev), 0, nf <= target_faces)
    vertices, faces32 = vertices.clone(), faces.to(torch.int32).contiguous()
    parent = torch.arange(nv, dtype=torch.int32, device=dev)
    quads, rounds = None, 0
    while faces32.shape[0] > target_faces and rounds < max_rounds:
        lists = round_lists(faces32, nv)
        if lists.edges.shape[0] == 0:
            break
        if quads is None:
            quads = quadrics(vertices, faces32, lists.vf_offsets, lists.vf_faces)
        fixed = mesh._pinned('decimate', pinned, nv, dev, lists.adj.boundary)
        target, cost, valid = edge_costs(vertices, quads, faces32, lists, fixed)
        perm, rank, need = candidate_ranks(cost, valid, faces32.shape[0], target_faces, fraction)
        apply = applied_edges(edge_select(rank, lists, nv), perm, need)
        if int(apply.sum()) == 0:                                           # the one copy of the round: no edge is valid
            break
        dead = collapse(vertices, quads, parent, faces32, lists.edges, apply, target)
        faces32 = faces32[dead == 0]
        rounds += 1
    root = parent.long()
    while True:                                                             # a vertex may have been merged into one that was merged later
        up = root[root]
        if torch.equal(up, root):
            break
        root = up
    faces = faces32.long()
    used = torch.zeros([nv], dtype=torch.bool, device=dev)
    used[faces.reshape(-1)] = True
    remap = torch.cumsum(used, 0) - 1
    vertex_map = torch.where(used[root], remap[root], torch.full_like(root, -1))
    return Decimation(vertices[used], remap[faces], vertex_map, rounds, faces.shape[0] <= target_faces)


def decimate_to(vertices, faces, tolerance, spacing=None, fraction=0.25):
    """``decimate`` with its target picked from a tolerance, ``mesh.simplify_to``'s contract: (vertices', faces', target_faces, agreement).  The targets
    are the ladder floor(T / 2^(i / 2)), i = 1, 2, ... while they stay at 4 faces or more (at most 40 rungs): rung 1 is tried, then a bisection over the
    rung index looks for the coarsest rung whose result keeps the sampled symmetric Hausdorff distance to the input (``geometry.compare`` at ``spacing``,
    default the input's diagonal over 512) at or below ``tolerance``.  The only promise is the post-condition: the mesh that comes back met the
    tolerance as measured, ``agreement`` being that measurement (A = the input), and the next rung tried did not.  If the first rung fails (or the mesh
    is too small for a ladder) the input comes back unchanged with target_faces None (and that rung's agreement, or None)."""
    from . import geometry                                                 # (geometry imports mesh, which imports this module on demand)
    tolerance = float(tolerance)
    if not (tolerance > 0.0 and math.isfinite(tolerance)):
        raise ValueError(f'decimate_to: tolerance must be positive and finite, got {tolerance}')
    vertices = mesh._mesh_vertices('decimate_to', vertices)
    faces = mesh._mesh_faces('decimate_to', faces, vertices.shape[0]).to(vertices.device)
    nf = faces.shape[0]
    targets = [int(nf / 2.0 ** (i / 2)) for i in range(1, DECIMATE_RUNGS + 1)]
    targets = [t for t in targets if t >= 4]
    if not targets:
        return vertices, faces, None, None
    spacing = geometry.diagonal(vertices) / 512 if spacing is None else float(spacing)

    def rung(i):
        out = decimate(vertices, faces, targets[i], fraction)
        agreement = geometry.compare(vertices, faces, out.vertices, out.faces, spacing, (tolerance,))
        return bool(agreement.hausdorff <= tolerance), (out.vertices, out.faces, targets[i], agreement)

    ok, best = rung(0)
    if not ok:
        return vertices, faces, None, best[3]
    passed, failed = 0, len(targets)
    while failed - passed > 1:
        middle = (passed + failed) // 2
        ok, result = rung(middle)
        if ok:
            passed, best = middle, result
        else:
            failed = middle
    return best
