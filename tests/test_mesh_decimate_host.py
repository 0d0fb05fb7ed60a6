"""pix2pix3d_amd.decimate on CPU tensors: the torch formulation against the plain-Python loop of decimate_cases.py, the invariants of the rules (what is
never touched, what stays closed and manifold, the face counts, the map), the error cases, ``decimate_to``'s post-condition, the ``target_faces=`` argument
of the mesh pipelines, and the quality of the result measured against ``mesh.simplify`` with ``geometry.compare``."""
import functools
import math

import pytest
import torch

import decimate_cases as dc
from pix2pix3d_amd import decimate, geometry, mesh


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _result(name):
    """``decimate`` of a small case on the CPU.  Do not modify."""
    v, f, target = dc.case(name)
    return decimate.decimate(v, f, target)


def _hausdorff(v, f, out_v, out_f, spacing):
    return float(geometry.compare(v, f, out_v, out_f, spacing).hausdorff)


@pytest.mark.parametrize('name', sorted(dc.SMALL_CASES))
def test_the_formulation_is_the_loop(name):
    v, f, target = dc.case(name)
    got, want = _result(name), dc.decimate_loop(v, f, target)
    assert torch.equal(got.faces, want[1]) and torch.equal(got.vertex_map, want[2])
    assert torch.equal(_bits(got.vertices), _bits(want[0]))
    assert (got.rounds, got.reached) == want[3:]
    assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int64 and got.vertex_map.dtype == torch.int64


def test_the_formulation_is_the_loop_with_pins_and_other_fractions():
    v, f = dc.icosphere(2)
    pinned = torch.zeros([len(v)], dtype=torch.bool)
    pinned[::7] = True
    for kw in (dict(pinned=pinned), dict(fraction=1.0), dict(fraction=0.01), dict(max_rounds=3)):
        got, want = decimate.decimate(v, f, 100, **kw), dc.decimate_loop(v, f, 100, **kw)
        assert torch.equal(got.faces, want[1]) and torch.equal(got.vertex_map, want[2]) and torch.equal(_bits(got.vertices), _bits(want[0]))
        assert (got.rounds, got.reached) == want[3:]
    kept = decimate.decimate(v, f, 100, pinned=pinned)
    assert (kept.vertex_map[pinned] >= 0).all() and torch.equal(_bits(kept.vertices[kept.vertex_map[pinned]]), _bits(v[pinned]))
    assert decimate.decimate(v, f, 100, max_rounds=3).rounds == 3 and not decimate.decimate(v, f, 100, max_rounds=3).reached


def test_a_tetrahedron_does_not_collapse():
    v, f, _ = dc.case('tetrahedron')
    out = _result('tetrahedron')
    assert not out.reached and out.rounds == 0 and torch.equal(out.faces, f) and torch.equal(_bits(out.vertices), _bits(v))
    assert torch.equal(out.vertex_map, torch.arange(4))


def test_an_octahedron_stops_at_six_faces():
    """8 -> 6 faces is one collapse and leaves a triangular bipyramid.  An edge between two equator vertices fails the link condition (three common
    neighbours); an edge from an apex (3 neighbours) to the equator (4) would leave a merged vertex with 3 neighbours, a tetrahedron, and is barred."""
    out = _result('octahedron')
    print(f'octahedron to 4: {len(out.faces)} faces after {out.rounds} rounds, reached {out.reached}')
    assert dc.is_closed_manifold(out.faces)
    assert len(out.faces) == 6 and not out.reached and out.rounds == 1


def test_a_fin_edge_and_the_boundary_are_never_touched():
    v, f, (a, b) = dc.fin()
    out = decimate.decimate(v, f, 30)
    tip = len(v) - 1
    for x in (a, b, tip):                                                   # the fin's edge is used by three faces; its tip is a boundary vertex
        assert out.vertex_map[x] >= 0 and torch.equal(_bits(out.vertices[out.vertex_map[x]]), _bits(v[x]))
    assert len({int(out.vertex_map[x]) for x in (a, b, tip)}) == 3 and len(out.faces) < len(f)
    fin_face = out.vertex_map[f[-1]]
    assert (out.faces == fin_face).all(1).any()


def test_the_plate_stays_planar_and_keeps_its_boundary():
    v, f, target = dc.case('plate')
    out = _result('plate')
    assert out.reached and target - 1 <= len(out.faces) <= target
    assert (out.vertices[:, 2] == 0.25).all()
    boundary = mesh.adjacency(f, len(v)).boundary
    assert (out.vertex_map[boundary] >= 0).all() and torch.equal(_bits(out.vertices[out.vertex_map[boundary]]), _bits(v[boundary]))
    assert int(mesh.adjacency(out.faces, len(out.vertices)).boundary.sum()) == int(boundary.sum())


@pytest.mark.parametrize('name', dc.CLOSED)
def test_closed_inputs_come_out_closed_and_manifold(name):
    v, f, _ = dc.case(name)
    assert dc.is_closed_manifold(f) and dc.is_closed_manifold(_result(name).faces)


@pytest.mark.parametrize('name', sorted(dc.SMALL_CASES))
def test_counts_rounds_and_the_map(name):
    v, f, target = dc.case(name)
    out = _result(name)
    assert out.reached == (len(out.faces) <= target) and len(out.faces) >= min(target - 1, len(f))
    assert out.rounds <= decimate.default_max_rounds(len(f)) == 16 * math.ceil(math.log2(len(f))) + 64
    used = torch.zeros([len(out.vertices)], dtype=torch.bool)
    used[out.faces.reshape(-1)] = True
    assert used.all() and out.vertex_map.shape == (len(v),)
    survivors = out.vertex_map[out.vertex_map >= 0]
    assert set(survivors.tolist()) == set(range(len(out.vertices)))
    # a face of the input either became a face of the output under the map or lost a corner to a merge
    mapped = out.vertex_map[f]
    alive = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2]) & (mapped >= 0).all(1)
    assert torch.equal(mapped[alive], out.faces)


def test_the_zero_area_faces_add_nothing_and_go():
    v, f, target = dc.case('zero_area')
    out = _result('zero_area')
    assert out.rounds >= 1 and ((out.faces[:, 0] != out.faces[:, 1]) & (out.faces[:, 1] != out.faces[:, 2])).all()
    lists = decimate.round_lists(f.to(torch.int32), len(v))
    q = decimate.quadrics(v, f.to(torch.int32), lists.vf_offsets, lists.vf_faces)
    q0 = decimate.quadrics(v, f[:-2].to(torch.int32), *decimate.vertex_faces(f[:-2], len(v)))
    assert torch.equal(q, q0) and torch.isfinite(q).all()


def test_errors_and_empty_meshes():
    v, f = dc.octahedron()
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError):
            decimate.decimate(v, f, bad)
    for fraction in (0.0, 1.5, float('nan')):
        with pytest.raises(ValueError):
            decimate.decimate(v, f, 4, fraction=fraction)
    with pytest.raises(ValueError):
        decimate.decimate(v, f + 1, 4)
    with pytest.raises(ValueError):
        decimate.decimate(v.clone().index_put_((torch.tensor(0), torch.tensor(0)), torch.tensor(float('inf'))), f, 4)
    with pytest.raises(ValueError):
        decimate.decimate(v, f, 4, pinned=torch.zeros([5], dtype=torch.bool))
    with pytest.raises(ValueError):
        decimate.decimate(v, f, 4, max_rounds=-1)
    with pytest.raises(ValueError):
        decimate.decimate_to(v, f, 0.0)
    out = decimate.decimate(v, f[:0], 4)
    assert out.reached and out.rounds == 0 and torch.equal(out.vertices, v) and len(out.faces) == 0 and torch.equal(out.vertex_map, torch.arange(6))
    out = decimate.decimate(v[:0], f[:0], 0)
    assert out.reached and out.vertices.shape == (0, 3) and out.faces.shape == (0, 3) and out.vertex_map.shape == (0,)
    out = decimate.decimate(v, f, 8)                                        # already there: nothing runs, the input's bytes come back
    assert out.reached and out.rounds == 0 and torch.equal(out.faces, f) and torch.equal(_bits(out.vertices), _bits(v))
    assert decimate.decimate(v, f, 4, max_rounds=0).rounds == 0


def test_decimate_to_keeps_its_promise():
    v, f = dc.icosphere(2)
    diagonal = geometry.diagonal(v)
    spacing = diagonal / 32
    targets = {}
    for tolerance in (0.04 * diagonal, 0.01 * diagonal):
        out_v, out_f, target, agreement = decimate.decimate_to(v, f, tolerance, spacing)
        assert target is not None and len(out_f) <= target < len(f) and float(agreement.hausdorff) <= tolerance
        assert float(agreement.hausdorff) == _hausdorff(v, f, out_v, out_f, spacing)
        again = decimate.decimate(v, f, target)
        assert torch.equal(again.faces, out_f) and torch.equal(_bits(again.vertices), _bits(out_v))
        targets[tolerance] = target
    assert targets[0.04 * diagonal] < targets[0.01 * diagonal]
    out_v, out_f, target, agreement = decimate.decimate_to(v, f, 1e-9 * diagonal, spacing)      # the first rung already fails
    assert target is None and torch.equal(out_f, f) and torch.equal(_bits(out_v), _bits(v)) and float(agreement.hausdorff) > 1e-9 * diagonal
    assert decimate.decimate_to(*dc.tetrahedron(), 1.0)[2:] == (None, None)      # four faces: no ladder


# ---- quality, against mesh.simplify: never against the code under test ------------------------------------------------------------------------
def _simplify_with_at_least(v, f, n_faces):
    """``mesh.simplify`` at the coarsest cell of the ladder 0.97^i diagonal / 2 that yields at least ``n_faces`` faces."""
    diagonal = geometry.diagonal(v)
    for i in range(400):
        out_v, out_f = mesh.simplify(v, f, 0.97 ** i * diagonal / 2)
        if len(out_f) >= n_faces:
            return out_v, out_f
    raise AssertionError('the ladder never reached the face count')


def test_the_cube_keeps_its_surface():
    v, f = dc.cube(16)
    out = decimate.decimate(v, f, 12)
    diagonal = geometry.diagonal(v)
    distance = _hausdorff(v, f, out.vertices, out.faces, diagonal / 128)
    print(f'cube 16: {len(f)} -> {len(out.faces)} faces in {out.rounds} rounds, sampled symmetric Hausdorff {distance:.3g} (diagonal {diagonal:.4g})')
    assert out.reached and len(out.faces) == 12 and dc.is_closed_manifold(out.faces)
    assert distance <= 1e-6 * diagonal


@pytest.mark.parametrize('target', [320, 160])
def test_the_icosphere_beats_clustering(target):
    v, f = dc.icosphere(3)
    out = decimate.decimate(v, f, target)
    assert out.reached and dc.is_closed_manifold(out.faces)
    sv, sf = _simplify_with_at_least(v, f, len(out.faces))
    spacing = geometry.diagonal(v) / 128
    ours, theirs = _hausdorff(v, f, out.vertices, out.faces, spacing), _hausdorff(v, f, sv, sf, spacing)
    print(f'icosphere 3: {len(f)} -> {len(out.faces)} faces in {out.rounds} rounds: Hausdorff {ours:.4g}; simplify at {len(sf)} faces: {theirs:.4g}; '
          f'ratio {theirs / ours:.3g}')
    assert ours < theirs


# ---- the pipelines ----------------------------------------------------------------------------------------------------------------------
def test_clean_geometry_takes_a_face_target(monkeypatch):
    v, f = dc.icosphere(2)
    monkeypatch.setattr(mesh.shape, 'extract_geometry', lambda G, ws, resolution, threshold, **kw: (v, f))
    base = mesh._clean_geometry(None, None, 16, 0.0, None, 1, None)
    assert torch.equal(base[0], v) and torch.equal(base[1], f)
    got = mesh._clean_geometry(None, None, 16, 0.0, 1, 1, None, target_faces=80)
    want = decimate.decimate(v, f, 80)
    assert torch.equal(got[1], want.faces) and torch.equal(_bits(got[0]), _bits(want.vertices))
    for clash in (dict(cell=0.1), dict(tolerance=0.1)):
        with pytest.raises(ValueError):
            mesh._clean_geometry(None, None, 16, 0.0, None, 1, clash.get('cell'), clash.get('tolerance'), target_faces=80)
