"""Shared by tests/test_geometry_host.py and tests/test_geometry_gpu.py: plain-Python restatements of the "mesh distances" section of include/p3d_hip.h (one Python
float operation per rounding: Python floats are IEEE doubles), the exact distance in fractions.Fraction, and the meshes and point sets
of the cases.  Nothing here calls pix2pix3d_amd.geometry's own formulations."""
import functools
import math
from fractions import Fraction

import torch

from pix2pix3d_amd import shape
from test_mesh_cleanup_host import spheres_field

INF = math.inf


# ---- include/p3d_hip.h ("mesh distances") in Python floats ------------------------------------------------------------------------------------
def dot(u, v):
    s = u[0] * v[0]
    s = s + u[1] * v[1]
    s = s + u[2] * v[2]
    return s


def sub(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def seg_d2(p, a, b):
    e, r = sub(b, a), sub(p, a)
    den, num = dot(e, e), dot(r, e)
    t = num / den if den > 0 else 0.0
    t = min(max(t, 0.0), 1.0)
    q = (r[0] - t * e[0], r[1] - t * e[1], r[2] - t * e[2])
    return dot(q, q)


def tri_d2(p, a, b, c):
    s = min(min(seg_d2(p, a, b), seg_d2(p, b, c)), seg_d2(p, c, a))
    e1, e2 = sub(b, a), sub(c, a)
    n = cross(e1, e2)
    nn = dot(n, n)
    ra, rb, rc = sub(p, a), sub(p, b), sub(p, c)
    wc = dot(cross(e1, ra), n)
    wa = dot(cross(sub(c, b), rb), n)
    wb = dot(cross(sub(a, c), rc), n)
    h = dot(ra, n)
    plane = (h * h) / nn if nn > 0 and wa >= 0 and wb >= 0 and wc >= 0 else s
    m = min(s, plane)
    g = tuple(max(max(min(a[k], b[k], c[k]) - p[k], p[k] - max(a[k], b[k], c[k])), 0.0) for k in range(3))
    return max(m, dot(g, g))


def _rows(t):
    """A float32 / integer tensor as rows of Python numbers (a float32 becomes the double of the same value)."""
    return [tuple(r) for r in t.double().tolist()] if t.is_floating_point() else [tuple(r) for r in t.tolist()]


def valid_faces(vertices, faces):
    """[(face id, a, b, c)] of the faces with indices in range and finite corners, ascending."""
    v, out = _rows(vertices), []
    for t, idx in enumerate(_rows(faces)):
        if all(0 <= i < len(v) for i in idx) and all(math.isfinite(x) for i in idx for x in v[i]):
            out.append((t, v[idx[0]], v[idx[1]], v[idx[2]]))
    return out


def closest_loop(points, vertices, faces):
    """The definition as a double loop: (d2 float64 [N], face int64 [N])."""
    tris = valid_faces(vertices, faces)
    d2, face = [], []
    for p in _rows(points):
        best, best_id = INF, -1
        if all(math.isfinite(x) for x in p):
            for t, a, b, c in tris:                                       # ascending ids and a strict <: the smallest id wins a tie
                d = tri_d2(p, a, b, c)
                if d < best:
                    best, best_id = d, t
        d2.append(best)
        face.append(best_id)
    return torch.tensor(d2, dtype=torch.float64), torch.tensor(face, dtype=torch.int64)


def samples_loop(vertices, faces, spacing, k_max):
    """surface_samples face by face: (points float32 [N, 3], face int64 [N], capped int)."""
    s2 = spacing * spacing
    pts, ids, capped = [], [], 0
    for t, a, b, c in valid_faces(vertices, faces):
        l2 = max(max(dot(sub(b, a), sub(b, a)), dot(sub(c, b), sub(c, b))), dot(sub(a, c), sub(a, c)))
        k = next((k for k in range(1, k_max + 1) if float(k * k) * s2 >= l2), None)
        if k is None:
            k, capped = k_max, capped + 1
        cells = [(3 * i + 1, 3 * j + 1) for i in range(k) for j in range(k - i)] + [(3 * i + 2, 3 * j + 2) for i in range(k - 1) for j in range(k - 1 - i)]
        assert len(cells) == k * k
        for n0, n1 in cells:
            n2 = 3 * k - n0 - n1
            row = []
            for x in range(3):
                s = float(n0) * a[x]
                s = s + float(n1) * b[x]
                s = s + float(n2) * c[x]
                row.append(s / float(3 * k))
            pts.append(row)
            ids.append(t)
    points = torch.tensor(pts, dtype=torch.float64).reshape(-1, 3).to(torch.float32)      # one rounding to fp32
    return points, torch.tensor(ids, dtype=torch.int64), capped


# ---- the exact distance -----------------------------------------------------------------------------------------------------
def exact_d2(p, a, b, c):
    """The squared distance from p to the closed triangle a b c in exact rational arithmetic (integer or Fraction coordinates)."""
    F = Fraction
    p, a, b, c = ([F(x) for x in q] for q in (p, a, b, c))
    fdot = lambda u, v: sum(x * y for x, y in zip(u, v))                  # noqa: E731
    fsub = lambda u, v: [x - y for x, y in zip(u, v)]                      # noqa: E731

    def seg(a, b):
        e, r = fsub(b, a), fsub(p, a)
        den = fdot(e, e)
        t = min(max(fdot(r, e) / den, F(0)), F(1)) if den > 0 else F(0)
        q = [x - t * y for x, y in zip(r, e)]
        return fdot(q, q)
    best = min(seg(a, b), seg(b, c), seg(c, a))
    e1, e2 = fsub(b, a), fsub(c, a)
    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    nn = fdot(n, n)
    if nn > 0:
        # barycentrics of the projection from the Gram matrix
        r = fsub(p, a)
        d11, d12, d22, r1, r2 = fdot(e1, e1), fdot(e1, e2), fdot(e2, e2), fdot(r, e1), fdot(r, e2)
        det = d11 * d22 - d12 * d12
        u, v = (d22 * r1 - d12 * r2) / det, (d11 * r2 - d12 * r1) / det
        if u >= 0 and v >= 0 and u + v <= 1:
            h = fdot(r, n)
            best = min(best, h * h / nn)
    return best


# ---- meshes and points --------------------------------------------------------------------------------------------------------
DEGENERATE_FACES = (((1, 2, 3), (1, 2, 3), (1, 2, 3)),                  # a point
                    ((0, 0, 0), (4, 2, -2), (4, 2, -2)),                 # two equal corners: a segment
                    ((-3, 1, 0), (5, 1, 0), (1, 1, 0)),                  # three collinear corners, the third between the others
                    ((0, 0, 0), (64, 1, 0), (-64, -1, 1)))              # a sliver


def soup(n_faces, seed, extent=10.0, size=0.7, n_vertices=None):
    """(vertices float32 [3 T, 3], faces int64 [T, 3]): T random small triangles scattered over a cube."""
    g = torch.Generator().manual_seed(seed)
    centre = (torch.rand([n_faces, 1, 3], generator=g) - 0.5) * extent
    v = (centre + (torch.rand([n_faces, 3, 3], generator=g) - 0.5) * size).reshape(-1, 3).float()
    return v, torch.arange(3 * n_faces).reshape(-1, 3)


def cloud(n, seed, extent=14.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand([n, 3], generator=g) - 0.5) * extent).float()


def spread_case():
    """Two clusters 10^3 units apart with duplicated faces, a NaN face and an out-of-range face; points in, between and far outside the
    clusters and one non-finite point: (points, vertices, faces)."""
    va, fa = soup(40, 11, extent=4.0)
    vb, fb = soup(30, 12, extent=4.0)
    vb = vb + torch.tensor([1000.0, 0.0, 0.0])
    v = torch.cat([va, vb, torch.tensor([[float('nan'), 0.0, 0.0]])])
    nan_vertex = len(v) - 1
    f = torch.cat([fa, fb + len(va), fa[5:9], fb[:3] + len(va),               # duplicates: the smaller id must win
                   torch.tensor([[0, 1, nan_vertex], [0, 1, len(v) + 5], [-1, 2, 3]])])
    g = torch.Generator().manual_seed(13)
    between = torch.stack([torch.linspace(-50, 1050, 40), torch.zeros(40), torch.zeros(40)], 1)
    far = (torch.rand([20, 3], generator=g) - 0.5) * 2e5
    on_faces = v[f[:8]].mean(1)                                            # centroids: distance about 0, ties between duplicates
    pts = torch.cat([cloud(60, 14, 6.0), cloud(60, 15, 6.0) + torch.tensor([1000.0, 0.0, 0.0]), between, far, on_faces,
                     torch.tensor([[0.0, float('inf'), 0.0], [float('nan')] * 3])]).float()
    return pts, v, f


def region_points(n, seed):
    """Points about the triangle of ``REGION_TRIANGLE`` that cover its seven Voronoi regions, its plane, edges and vertices."""
    g = torch.Generator().manual_seed(seed)
    a, b, c = (torch.tensor(x, dtype=torch.float32) for x in REGION_TRIANGLE)
    w = torch.rand([n, 3], generator=g) * 3.0 - 1.0                        # barycentrics in [-1, 2]: all seven regions
    w = w / w.sum(1, keepdim=True).clamp(min=0.2)
    pts = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
    lift = torch.randn([n, 1], generator=g) * torch.tensor([0.0, 0.0, 1.0])
    lift[: n // 4] = 0.0                                                   # a quarter in the plane
    pts = pts + lift
    pts[:3] = torch.stack([a, b, c])                                       # on the vertices
    pts[3:6] = torch.stack([(a + b) / 2, (b + c) / 2, (c + a) / 2])        # on the edges
    return pts.float()


REGION_TRIANGLE = ((0.0, 0.0, 0.0), (3.0, 0.0, 0.0), (1.0, 2.0, 0.0))


@functools.lru_cache(maxsize=None)
def sphere_mesh(radius, n=48, centre=(23.5, 23.5, 23.5)):
    """(vertices, faces) of one marching-cubes sphere on an n^3 lattice, index space.  Do not modify."""
    return shape.marching_cubes(spheres_field(which=(0,), n=n, spheres=((centre, radius),)), 0.0)


@functools.lru_cache(maxsize=None)
def small_sphere(radius):
    """A sphere on a 24^3 lattice about (11.5, 11.5, 11.5): small enough for the all-pairs definition.  Do not modify."""
    return sphere_mesh(radius, 24, (11.5, 11.5, 11.5))
