"""Shared by tests/test_mesh_decimate_host.py and tests/test_mesh_decimate_gpu.py: the meshes of the cases, built analytically, and a plain-Python loop
that restates the rules of csrc/mesh/p3d_mesh.h (one Python float operation per rounding: Python floats are IEEE doubles; lists
and dicts instead of sorts).  Nothing here calls pix2pix3d_amd.decimate's own formulations."""
import functools
import math
import struct

import torch

INF = math.inf
NO_RANK = 2 ** 31 - 1


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------
def _mesh(vertices, faces):
    return torch.tensor(vertices, dtype=torch.float32).reshape(-1, 3), torch.tensor(faces, dtype=torch.int64).reshape(-1, 3)


def tetrahedron():
    return _mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], [(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)])


_OCTA_V = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
_OCTA_F = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]


def octahedron():
    return _mesh(_OCTA_V, _OCTA_F)


def two_octahedra():
    v, f = octahedron()
    return torch.cat([v, v * 0.5 + torch.tensor([4.0, 0.25, 0.0])]), torch.cat([f, f + len(v)])


@functools.lru_cache(maxsize=None)
def cube(n):
    """A closed cube of edge n with n x n quads a side, integer coordinates, outward normals: 6 n^2 + 2 vertices, 12 n^2 faces.  Do not modify."""
    index, vertices, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(vertices)
            vertices.append(p)
        return index[p]
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def corner(di, dj):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        return vid(tuple(p))
                    a, b, c, d = corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)
                    faces += [(a, b, c), (a, c, d)] if side else [(a, c, b), (a, d, c)]
    return _mesh(vertices, faces)


def plate(n=9):
    """An n x n grid of vertices in the plane z = 0.25 with a boundary: 2 (n - 1)^2 faces."""
    vertices = [(i, j, 0.25) for j in range(n) for i in range(n)]
    faces = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            faces += [(a, a + 1, a + n + 1), (a, a + n + 1, a + n)]
    return _mesh(vertices, faces)


@functools.lru_cache(maxsize=None)
def icosphere(subdivisions, axes=(1.0, 0.6, 0.35)):
    """The squashed icosphere: 20 * 4^s faces on the ellipsoid with these semi-axes, outward normals.  Do not modify."""
    t = (1 + math.sqrt(5)) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    unit = lambda p: tuple(x / math.sqrt(sum(y * y for y in p)) for x in p)      # noqa: E731
    v = [unit(p) for p in v]
    for _ in range(subdivisions):
        middle, out = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in middle:
                middle[key] = len(v)
                v.append(unit(tuple((x + y) / 2 for x, y in zip(v[a], v[b]))))
            return middle[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    vertices, faces = _mesh(v, f)
    return vertices * torch.tensor(axes, dtype=torch.float32), faces


def fin():
    """The subdivision-1 icosphere with a third face on the edge of its first face (a fin on a new vertex), and that vertex's index."""
    v, f = icosphere(1)
    a, b = int(f[0, 0]), int(f[0, 1])
    tip = (v[a] + v[b]) * 0.9
    return torch.cat([v, tip[None]]), torch.cat([f, torch.tensor([[a, b, len(v)]])]), (a, b)


def zero_area():
    """The subdivision-1 icosphere with one face repeated as a sliver of no area (two of its corners and the middle of them: a T-junction face)."""
    v, f = icosphere(1)
    a, b = int(f[3, 0]), int(f[3, 1])
    return torch.cat([v, ((v[a] + v[b]) * 0.5)[None]]), torch.cat([f, torch.tensor([[a, b, b]]), torch.tensor([[b, a, a]])])


SMALL_CASES = {'tetrahedron': (tetrahedron, 2), 'octahedron': (octahedron, 4), 'cube4': (lambda: cube(4), 12), 'plate': (plate, 40),
               'icosphere2': (lambda: icosphere(2), 80), 'two_octahedra': (two_octahedra, 8), 'fin': (lambda: fin()[:2], 30),
               'zero_area': (zero_area, 30)}
CLOSED = ('tetrahedron', 'octahedron', 'cube4', 'icosphere2', 'two_octahedra')


def case(name):
    """(vertices, faces, target_faces) of a small case."""
    make, target = SMALL_CASES[name]
    return make() + (target,)


# ---- the rules in Python ------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return struct.unpack('f', struct.pack('f', x))[0]


def sub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def dot(u, v):
    s = u[0] * v[0]
    s = s + u[1] * v[1]
    s = s + u[2] * v[2]
    return s


def cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def normal(a, b, c):
    return cross(sub(b, a), sub(c, a))


def face_quadric(a, b, c):
    n = normal(a, b, c)
    nn = dot(n, n)
    if nn == 0:
        return None
    length = math.sqrt(nn)
    h = (n[0] / length, n[1] / length, n[2] / length)
    p = h + (-dot(h, a),)
    w = length * 0.5
    return [w * (p[r] * p[c2]) for r in range(4) for c2 in range(r, 4)]


def cost_of(q, x):
    rows = []
    for i, j, k, l in ((0, 1, 2, 3), (1, 4, 5, 6), (2, 5, 7, 8), (3, 6, 8, 9)):
        r = q[i] * x[0]
        r = r + q[j] * x[1]
        r = r + q[k] * x[2]
        rows.append(r + q[l])
    c = x[0] * rows[0]
    c = c + x[1] * rows[1]
    c = c + x[2] * rows[2]
    c = c + rows[3]
    return c if c > 0 else 0.0


def mix(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    return x ^ (x >> 16)


def target_and_cost(q, pa, pb):
    mid = tuple((pa[k] + pb[k]) * 0.5 for k in range(3))
    candidates = [pa, pb, mid]
    c00, c01, c02 = q[4] * q[7] - q[5] * q[5], q[2] * q[5] - q[1] * q[7], q[1] * q[5] - q[2] * q[4]
    c11, c12, c22 = q[0] * q[7] - q[2] * q[2], q[1] * q[2] - q[0] * q[5], q[0] * q[4] - q[1] * q[1]
    det = q[0] * c00
    det = det + q[1] * c01
    det = det + q[2] * c02
    m = max(abs(q[k]) for k in (0, 1, 2, 4, 5, 7))
    bound = m * m
    bound = bound * m
    bound = bound * 2.0 ** -20
    if abs(det) > bound:
        s = []
        for x, y, z in ((c00, c01, c02), (c01, c11, c12), (c02, c12, c22)):
            r = x * q[3]
            r = r + y * q[6]
            r = r + z * q[8]
            s.append((-r) / det)
        off, ab = sub(s, mid), sub(pb, pa)
        if dot(off, off) <= dot(ab, ab) * 4.0:
            candidates.append(tuple(s))
    best, best_cost = None, INF
    for x in candidates:
        c = cost_of(q, x)
        if best is None or c < best_cost:
            best, best_cost = x, c
    return best, best_cost


def decimate_loop(vertices, faces, target_faces, fraction=0.25, max_rounds=None, pinned=None):
    """Rules 1 - 9, as DESIGN.md section 2.1aa numbers them, with loops: (vertices float32 [V', 3], faces int64 [T', 3], vertex_map int64 [V], rounds, reached)."""
    pos = [tuple(r) for r in vertices.double().tolist()]
    tris = [tuple(r) for r in faces.tolist()]
    nv = len(pos)
    pinned = [False] * nv if pinned is None else [bool(x) for x in pinned.tolist()]
    if max_rounds is None:
        max_rounds = 16 * math.ceil(math.log2(max(len(tris), 1))) + 64
    parent = list(range(nv))
    # rule 1
    quads = [[0.0] * 10 for _ in range(nv)]
    for a, b, c in tris:                                                    # ascending face id at every vertex
        k = face_quadric(pos[a], pos[b], pos[c])
        if k is not None:
            for v in (a, b, c):                                             # a face that names a vertex twice adds twice: it has no area, so it adds nothing
                quads[v] = [x + y for x, y in zip(quads[v], k)]
    rounds = 0
    while len(tris) > target_faces and rounds < max_rounds and nv:
        # rule 2: the lists of the round
        nbrs, uses, of_vertex = [set() for _ in range(nv)], {}, [[] for _ in range(nv)]
        for t, tri in enumerate(tris):
            for k in range(3):
                of_vertex[tri[k]].append(t)                                 # (twice for a vertex named twice)
                a, b = tri[k], tri[(k + 1) % 3]
                if a != b:
                    nbrs[a].add(b)
                    nbrs[b].add(a)
                    uses[(min(a, b), max(a, b))] = uses.get((min(a, b), max(a, b)), 0) + 1
        boundary = [False] * nv
        for (a, b), n in uses.items():
            if n == 1:
                boundary[a] = boundary[b] = True
        edges = sorted(uses)
        if not edges:
            break
        # rules 3 and 4
        valid, target, cost = [], [], []
        for a, b in edges:
            ok = not (boundary[a] or boundary[b] or pinned[a] or pinned[b])
            thirds = []
            for t in of_vertex[a]:
                if b in tris[t]:
                    others = [x for x in tris[t] if x not in (a, b)]
                    thirds.append(others[0] if others else tris[t][2])
            ok = ok and len(thirds) == 2 and thirds[0] != thirds[1]
            common = sorted(nbrs[a] & nbrs[b])
            ok = ok and len(common) == 2 and common == sorted(thirds) and all(len(nbrs[c]) >= 4 for c in common)
            ok = ok and len(nbrs[a]) + len(nbrs[b]) - 4 >= 4                  # the merged vertex keeps at least 4 neighbours
            p, c = (0.0, 0.0, 0.0), INF
            if ok:
                best, c = target_and_cost([x + y for x, y in zip(quads[a], quads[b])], pos[a], pos[b])
                ok = c < INF
                p = tuple(_f32(x) for x in best)
            if ok:
                for v, other in ((a, b), (b, a)):
                    for t in of_vertex[v]:
                        tri = tris[t]
                        if other in tri:
                            continue
                        n0 = normal(*(pos[x] for x in tri))
                        nn0 = dot(n0, n0)
                        if not nn0 > 0:
                            continue
                        n1 = normal(*(p if x == v else pos[x] for x in tri))
                        nn1, d = dot(n1, n1), dot(n0, n1)
                        ok = ok and d > 0 and d * d >= (nn0 * nn1) * 0.0625
            valid.append(ok)
            target.append(p if ok else (0.0, 0.0, 0.0))
            cost.append(c if ok else INF)
        # rules 5 and 6
        ne = len(edges)
        order = sorted(range(ne), key=lambda e: (cost[e], mix(e)))
        rank = [0] * ne
        for r, e in enumerate(order):
            rank[e] = r
        n_valid = sum(valid)
        need = (len(tris) - target_faces + 1) // 2
        k = min(max(1, math.ceil(fraction * n_valid)), need)
        tau = cost[order[k - 1]]
        crank = [rank[e] if valid[e] and cost[e] <= tau else NO_RANK for e in range(ne)]
        # rule 7
        m1 = [NO_RANK] * nv
        for e, (a, b) in enumerate(edges):
            m1[a], m1[b] = min(m1[a], crank[e]), min(m1[b], crank[e])
        m2 = [min([m1[v]] + [m1[w] for w in nbrs[v]]) for v in range(nv)]
        winners = sorted((crank[e], e) for e, (a, b) in enumerate(edges) if crank[e] != NO_RANK and crank[e] == m2[a] == m2[b])
        if not winners:
            break
        # rule 8
        for _, e in winners[:need]:
            a, b = edges[e]
            pos[a] = target[e]
            quads[a] = [x + y for x, y in zip(quads[a], quads[b])]
            parent[b] = a
        tris = [tuple(parent[x] for x in tri) for tri in tris]
        tris = [tri for tri in tris if len(set(tri)) == 3]
        rounds += 1

    def root(v):
        while parent[v] != v:
            v = parent[v]
        return v
    used = sorted({x for tri in tris for x in tri})
    new = {v: i for i, v in enumerate(used)}
    if not len(faces) or not nv:
        return vertices.float(), faces.long(), torch.arange(nv), 0, len(faces) <= target_faces
    out_v = torch.tensor([pos[v] for v in used], dtype=torch.float64).reshape(-1, 3).float()
    out_f = torch.tensor([[new[x] for x in tri] for tri in tris], dtype=torch.int64).reshape(-1, 3)
    vertex_map = torch.tensor([new.get(root(v), -1) for v in range(nv)], dtype=torch.int64)
    return out_v, out_f, vertex_map, rounds, len(tris) <= target_faces


# ---- checks -------------------------------------------------------------------------------------------------------------------------------
def is_closed_manifold(faces):
    """Every directed edge occurs once, and its reverse once."""
    directed = {}
    for a, b, c in faces.tolist():
        if len({a, b, c}) != 3:
            return False
        for e in ((a, b), (b, c), (c, a)):
            directed[e] = directed.get(e, 0) + 1
    return all(n == 1 and directed.get((b, a), 0) == 1 for (a, b), n in directed.items())
