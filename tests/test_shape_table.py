"""The generated marching-cubes case table (pix2pix3d_amd/mc_table.py, csrc/mc_tables.h)."""
import os

import pytest

import pix2pix3d_amd.shape  # noqa: F401  (the feature this table belongs to)
from pix2pix3d_amd import mc_table as M


def _crossed(case):
    ins = [(case >> c) & 1 for c in range(8)]
    return {e for e in range(12) if ins[M.edge_ends(e)[0]] != ins[M.edge_ends(e)[1]]}


def _face_rule(case, face):
    """The face rule restated: undirected pairs of crossed edges on one face.  Two crossings: one pair.  Four (diagonal corners inside):
    the two edges around each inside corner."""
    _, _, corners, edges = face
    ins = [(case >> c) & 1 for c in range(8)]
    crossed = [e for e in edges if e in _crossed(case)]
    if len(crossed) == 2:
        return {frozenset(crossed)}
    if len(crossed) == 4:
        return {frozenset(e for e in crossed if c in M.edge_ends(e)) for c in corners if ins[c]}
    assert not crossed
    return set()


def _boundary(tris):
    """Directed edges of a triangle list that are not cancelled by their reverse: the loops the fans were built from."""
    directed = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
    out = [d for d in directed if (d[1], d[0]) not in directed]
    assert len(out) == len(set(out))
    return set(out)


@pytest.mark.parametrize('case', range(256))
def test_case_uses_exactly_its_crossed_edges(case):
    tris = M.triangles()[case]
    used = {e for t in tris for e in t}
    assert used == _crossed(case)
    assert len(tris) <= M.MAX_TRIANGLES
    assert all(len(set(t)) == 3 for t in tris)


def test_segments_on_every_face_follow_the_face_rule():
    for case in range(256):
        bnd = _boundary(M.triangles()[case])
        on_faces = set()
        for f in M.faces():
            fe = set(f[3])
            segs = {d for d in bnd if d[0] in fe and d[1] in fe}
            assert {frozenset(d) for d in segs} == _face_rule(case, f), (case, f)
            assert segs == set(M.face_segments(case, f)), (case, f)
            on_faces |= segs
        assert on_faces == bnd, case                      # every boundary segment lies on a face


def test_no_chord_joins_two_vertices_of_one_face():
    # a chord of the fan between two vertices on one cube face could be the neighbour's chord too: the mesh would not be closed
    for case in range(256):
        tris = M.triangles()[case]
        bnd = {frozenset(d) for d in _boundary(tris)}
        chords = {frozenset((t[i], t[(i + 1) % 3])) for t in tris for i in range(3)} - bnd
        for c in chords:
            assert not any(c <= set(f[3]) for f in M.faces()), (case, sorted(c))


def test_complement_has_the_same_edges_reversed_where_no_face_is_ambiguous():
    # Without an ambiguous face, inside and outside swap roles exactly: the same loops, opposite orientation.
    for case in range(256):
        if any(len([e for e in f[3] if e in _crossed(case)]) == 4 for f in M.faces()):
            continue
        a = _boundary(M.triangles()[case])
        b = _boundary(M.triangles()[255 - case])
        assert a == {(y, x) for x, y in b}, case


def test_largest_cube_and_committed_header_match_the_generator():
    assert M.max_triangles() == M.MAX_TRIANGLES
    with open(M.HEADER_PATH) as f:
        committed = f.read()
    assert committed == M.emit_header(), 'csrc/mc_tables.h is stale: run python -m pix2pix3d_amd.mc_table'
    assert os.path.basename(M.HEADER_PATH) == 'mc_tables.h'
