"""The marching-cubes case table, generated from first principles (no table is copied from anywhere).

A cube's corners are numbered c = dx + 2 dy + 4 dz, where (dx, dy, dz) is the corner's offset along the field's axes (0, 1, 2); its case
is sum_c inside(c) << c, with a corner inside when its value is strictly above the threshold.  An edge is (lower corner c, axis a); the
twelve are listed in EDGES, ordered by corner, then axis.  For every case the table lists triangles as triples of edge ids:

1. the crossed edges are those whose two ends differ in inside-ness;
2. on each of the six cube faces the crossed edges are paired into segments.  On an ambiguous face (two diagonal corners inside, the
   other two outside) each inside corner is cut off on its own: the two inside corners are SEPARATED.  Two cubes that share a face see
   the same four corners, so they pair the same edges and the surface is watertight;
3. each segment is oriented so that, seen from outside the cube, the face's inside part lies on its right; the segments then chain
   into closed loops whose right-hand normal points from inside to outside;
4. each loop, started at its lowest edge id, is fan-triangulated: (l0, l_i, l_i+1) — from the first vertex l0 in loop order whose
   fan has no chord between two vertices on one cube face.  Such a chord could also be a chord of the neighbour across that face
   (an ambiguous face carries four vertices); without one, every mesh edge inside a cube belongs to that cube alone and every edge
   on a face is one face segment, used once in each direction by the two cubes: the mesh is closed and oriented.

This is not Lorensen and Cline's original table: its ambiguous faces are resolved by the rule above, so its surfaces differ from
PyMCubes' on those cases on purpose.  ``python -m pix2pix3d_amd.mc_table`` rewrites csrc/mc_tables.h, which the kernels of
csrc/shape.hip read; tests/test_shape_table.py checks that the committed header is what this module emits.
"""
import functools
import os

CORNERS = tuple((c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8))
EDGES = tuple((c, a) for c in range(8) for a in range(3) if not (c >> a) & 1)
HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', 'mc_tables.h')


def edge_ends(e):
    c, a = EDGES[e]
    return c, c | (1 << a)


def faces():
    """The six cube faces as (axis, side, corners, edges): the face where the axis-`axis` offset equals `side`."""
    out = []
    for a in range(3):
        for s in range(2):
            corners = tuple(c for c in range(8) if ((c >> a) & 1) == s)
            edges = tuple(e for e, (c, ea) in enumerate(EDGES) if ea != a and ((c >> a) & 1) == s)
            out.append((a, s, corners, edges))
    return tuple(out)


def _sub(p, q): return tuple(x - y for x, y in zip(p, q))
def _cross(p, q): return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])
def _dot(p, q): return sum(x * y for x, y in zip(p, q))
def _mean(ps): return tuple(sum(p[i] for p in ps) / len(ps) for i in range(3))


def _midpoint(e):
    c0, c1 = edge_ends(e)
    return _mean([CORNERS[c0], CORNERS[c1]])


def face_segments(case, face):
    """The directed segments (edge id, edge id) that the face rule puts on one face for a case."""
    a, s, corners, edges = face
    inside = [(case >> c) & 1 for c in range(8)]
    crossed = [e for e in edges if inside[edge_ends(e)[0]] != inside[edge_ends(e)[1]]]
    ins = [c for c in corners if inside[c]]
    outs = [c for c in corners if not inside[c]]
    if not crossed:
        return []
    if len(crossed) == 2:                                  # one inside region on this face: one segment, inside -> outside along g
        pairs = [(crossed[0], crossed[1], _sub(_mean([CORNERS[c] for c in outs]), _mean([CORNERS[c] for c in ins])))]
    else:                                                  # ambiguous face: cut each inside corner off on its own
        assert len(crossed) == 4 and len(ins) == 2
        centre = _mean([CORNERS[c] for c in corners])
        pairs = []
        for c in ins:
            around = [e for e in crossed if c in edge_ends(e)]
            assert len(around) == 2
            pairs.append((around[0], around[1], _sub(centre, CORNERS[c])))
    normal = tuple((1 if s else -1) * (1 if i == a else 0) for i in range(3))    # the face's normal, out of the cube
    segs = []
    for e0, e1, g in pairs:
        d = _sub(_midpoint(e1), _midpoint(e0))
        side = _dot(_cross(g, d), normal)
        assert side != 0
        segs.append((e0, e1) if side < 0 else (e1, e0))
    return segs


def case_loops(case):
    """The closed, oriented edge loops of a case, each starting at its lowest edge id, in the order of those ids."""
    nxt = {}
    for f in faces():
        for e0, e1 in face_segments(case, f):
            assert e0 not in nxt, (case, e0)               # every crossed edge starts exactly one segment ...
            nxt[e0] = e1
    assert sorted(nxt) == sorted(nxt.values()), case       # ... and ends exactly one
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop = [e]
        seen.add(e)
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
            seen.add(loop[-1])
        loops.append(loop)
    return loops


def _on_one_face(e0, e1):
    return any(e0 in f[3] and e1 in f[3] for f in faces())


def fan(loop):
    """The loop rotated to the first apex whose fan chords (l0, l_i), 2 <= i <= L-2, never join two vertices of one cube face."""
    for r in range(len(loop)):
        rot = loop[r:] + loop[:r]
        if not any(_on_one_face(rot[0], rot[i]) for i in range(2, len(rot) - 1)):
            return rot
    raise AssertionError(f'no fan apex for loop {loop}')


@functools.lru_cache(maxsize=None)
def triangles():
    """Per case, the tuple of triangles (edge id triples) in table order."""
    out = []
    for case in range(256):
        tris = []
        for loop in case_loops(case):
            assert len(loop) >= 3
            rot = fan(loop)
            tris += [(rot[0], rot[i], rot[i + 1]) for i in range(1, len(rot) - 1)]
        out.append(tuple(tris))
    return tuple(out)


def max_triangles():
    return max(len(t) for t in triangles())


MAX_TRIANGLES = 5          # the largest number of triangles one cube holds; the kernels size their work from it


def _check():
    m = max_triangles()
    assert m == MAX_TRIANGLES, f'a cube holds up to {m} triangles, not {MAX_TRIANGLES}'


def emit_header():
    """The text of csrc/mc_tables.h."""
    _check()
    tris = triangles()
    lines = ['// Marching-cubes case table: GENERATED by pix2pix3d_amd/mc_table.py (python -m pix2pix3d_amd.mc_table), do not edit.',
             '// Corner c = dx + 2 dy + 4 dz (offsets along the field axes 0, 1, 2); case = sum_c (u_c > threshold) << c.',
             '// Edge e = (kMcEdgeCorner[e], kMcEdgeAxis[e]): its lower corner and its axis.  kMcTris[case]: kMcTriCount[case] triangles of',
             '// three edge ids each (-1 beyond); ambiguous faces separate their two inside corners (see mc_table.py).',
             '#pragma once',
             '#include <stdint.h>',
             '',
             'namespace p3d {',
             '',
             f'constexpr int kMcMaxTris = {MAX_TRIANGLES};',
             '__constant__ int8_t kMcEdgeCorner[12] = {' + ', '.join(str(c) for c, _ in EDGES) + '};',
             '__constant__ int8_t kMcEdgeAxis[12] = {' + ', '.join(str(a) for _, a in EDGES) + '};',
             '__constant__ uint8_t kMcTriCount[256] = {']
    for r in range(0, 256, 32):
        lines.append('    ' + ', '.join(str(len(t)) for t in tris[r:r + 32]) + ',')
    lines.append('};')
    lines.append('__constant__ int8_t kMcTris[256][kMcMaxTris * 3] = {')
    for case, t in enumerate(tris):
        flat = [e for tri in t for e in tri] + [-1] * (3 * (MAX_TRIANGLES - len(t)))
        lines.append('    {' + ', '.join(str(e) for e in flat) + '},' + f'   // {case}')
    lines += ['};', '', '} // namespace p3d', '']
    return '\n'.join(lines)


if __name__ == '__main__':
    with open(HEADER_PATH, 'w') as f:
        f.write(emit_header())
    print(f'wrote {HEADER_PATH} (up to {max_triangles()} triangles per cube)')
