"""pix2pix3d_amd.decimate on the device: the kernels of csrc/mesh/mesh_decimate.hip against the CPU formulation bit for bit — whole decimations of every
case of decimate_cases.py (the subdivision-5 icosphere spans many work-groups and rounds), each entry point alone against its torch restatement,
offset and non-contiguous operands, the library's launch counter, and ``extract_mesh(target_faces=)`` on a seeded generator."""
import functools

import pytest
import torch

import decimate_cases as dc
from pix2pix3d_amd import decimate, mesh
from test_mesh_gpu import _median_mesh

pytestmark = pytest.mark.gpu

LARGE_CASES = {'cube16': (lambda: dc.cube(16), 12), 'icosphere3': (lambda: dc.icosphere(3), 160), 'icosphere5': (lambda: dc.icosphere(5), 2560)}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _case(name):
    if name in dc.SMALL_CASES:
        return dc.case(name)
    make, target = LARGE_CASES[name]
    return make() + (target,)


@functools.lru_cache(maxsize=None)
def _cpu_result(name):
    """``decimate`` of a case on the CPU.  Do not modify."""
    v, f, target = _case(name)
    return decimate.decimate(v, f, target)


def _assert_same(dev, cpu):
    assert dev.vertices.is_cuda and dev.faces.is_cuda and dev.vertex_map.is_cuda
    assert dev.vertices.dtype == torch.float32 and dev.faces.dtype == torch.int64 and dev.vertex_map.dtype == torch.int64
    assert (dev.rounds, dev.reached) == (cpu.rounds, cpu.reached)
    assert torch.equal(dev.faces.cpu(), cpu.faces) and torch.equal(dev.vertex_map.cpu(), cpu.vertex_map)
    assert torch.equal(_bits(dev.vertices.cpu()), _bits(cpu.vertices))


@pytest.mark.parametrize('name', sorted(dc.SMALL_CASES) + sorted(LARGE_CASES))
def test_decimate_matches_cpu(hip_lib, name):
    v, f, target = _case(name)
    cpu = _cpu_result(name)
    n0 = decimate.launch_count()
    dev = decimate.decimate(v.cuda(), f.cuda(), target)
    torch.cuda.synchronize()
    # the quadrics once, six launches per round that collapsed, and four (costs, select) for a last round in which no edge was valid
    stalled = not cpu.reached and cpu.rounds < decimate.default_max_rounds(len(f))
    assert decimate.launch_count() - n0 == 1 + decimate.LAUNCHES_PER_ROUND * cpu.rounds + (4 if stalled else 0)
    _assert_same(dev, cpu)
    if name in LARGE_CASES:
        assert cpu.reached and cpu.rounds > 20 and dc.is_closed_manifold(cpu.faces)


@functools.lru_cache(maxsize=None)
def _round_operands():
    """The operands of the first round of the subdivision-2 icosphere with every seventh vertex pinned, on the CPU.  Do not modify."""
    v, f = dc.icosphere(2)
    faces32 = f.to(torch.int32)
    lists = decimate.round_lists(faces32, len(v))
    fixed = lists.adj.boundary.to(torch.uint8)
    fixed[::7] = 1
    quads = decimate.quadrics(v, faces32, lists.vf_offsets, lists.vf_faces)
    target, cost, valid = decimate.edge_costs(v, quads, faces32, lists, fixed)
    perm, rank, need = decimate.candidate_ranks(cost, valid, len(f), 80, 0.25)
    win = decimate.edge_select(rank, lists, len(v))
    apply = decimate.applied_edges(win, perm, need)
    return v, faces32, lists, fixed, quads, target, cost, valid, rank, win, apply


def _cuda_lists(lists):
    return decimate.Round(mesh.Adjacency(*(t.cuda() for t in lists.adj)), *(t.cuda() for t in lists[1:]))


def test_quadrics_alone(hip_lib):
    v, faces32, lists, _, quads = _round_operands()[:5]
    n0 = decimate.launch_count()
    dev = decimate.quadrics(v.cuda(), faces32.cuda(), lists.vf_offsets.cuda(), lists.vf_faces.cuda())
    assert decimate.launch_count() == n0 + 1
    assert torch.equal(dev.cpu().view(torch.int64), quads.view(torch.int64)) and (quads[:, 9] > 0).all()


def test_edge_costs_alone(hip_lib):
    v, faces32, lists, fixed, quads, target, cost, valid = _round_operands()[:8]
    n0 = decimate.launch_count()
    dev = decimate.edge_costs(v.cuda(), quads.cuda(), faces32.cuda(), _cuda_lists(lists), fixed.cuda())
    assert decimate.launch_count() == n0 + 1
    assert torch.equal(dev[2].cpu(), valid) and 0 < int(valid.sum()) < len(valid)
    assert torch.equal(dev[1].cpu().view(torch.int64), cost.view(torch.int64)) and torch.equal(_bits(dev[0].cpu()), _bits(target))


def test_edge_select_alone(hip_lib):
    v, _, lists, _, _, _, _, _, rank, win, _ = _round_operands()
    n0 = decimate.launch_count()
    dev = decimate.edge_select(rank.cuda(), _cuda_lists(lists), len(v))
    assert decimate.launch_count() == n0 + 3
    assert torch.equal(dev.cpu(), win) and 1 < int(win.sum()) < int((rank != decimate.NO_RANK).sum())


def test_collapse_alone(hip_lib):
    v, faces32, lists, _, quads, target, _, _, _, _, apply = _round_operands()
    assert int(apply.sum()) > 1
    state = [v.clone(), quads.clone(), torch.arange(len(v), dtype=torch.int32), faces32.clone()]
    dead = decimate.collapse(*state, lists.edges, apply, target)
    on_device = [t.cuda() for t in (v, quads, torch.arange(len(v), dtype=torch.int32), faces32)]
    n0 = decimate.launch_count()
    dead_device = decimate.collapse(*on_device, lists.edges.cuda(), apply.cuda(), target.cuda())
    assert decimate.launch_count() == n0 + 2
    assert torch.equal(dead_device.cpu(), dead) and int(dead.sum()) == 2 * int(apply.sum())
    assert torch.equal(_bits(on_device[0].cpu()), _bits(state[0])) and torch.equal(on_device[1].cpu().view(torch.int64), state[1].view(torch.int64))
    assert torch.equal(on_device[2].cpu(), state[2]) and torch.equal(on_device[3].cpu(), state[3])
    assert not torch.equal(state[0], v) and not torch.equal(state[3], faces32)


def test_offset_and_strided_operands(hip_lib):
    v, f, target = _case('icosphere2')
    cpu = _cpu_result('icosphere2')
    wide = torch.full([len(v) + 3, 7], 1e9, device='cuda')
    wide[2:-1, 1:4] = v.cuda()
    faces = torch.full([3, 2 * len(f) + 1], -5, dtype=torch.int32, device='cuda')
    faces[:, 1::2] = f.cuda().to(torch.int32).t()
    pinned = torch.zeros([2 * len(v)], dtype=torch.bool, device='cuda')
    before = (wide.clone(), faces.clone())
    _assert_same(decimate.decimate(wide[2:-1, 1:4], faces[:, 1::2].t(), target, pinned=pinned[::2]), cpu)
    assert torch.equal(wide, before[0]) and torch.equal(faces, before[1])      # the inputs are left as they were


def test_extract_mesh_with_a_face_target(hip_lib):
    G, ws, thr = _median_mesh('seg2cat', 32)
    kw = dict(resolution=32, threshold=thr, n_frames=2, image_size=64, keep=1)
    v0, f0, _, _ = mesh.extract_mesh(G, ws, **kw)
    target = len(f0) // 4
    n0 = decimate.launch_count()
    v, f, colors, frames = mesh.extract_mesh(G, ws, target_faces=target, **kw)
    torch.cuda.synchronize()
    assert decimate.launch_count() > n0 and len(f0) > 400
    cpu = decimate.decimate(v0.cpu(), f0.cpu(), target)
    assert torch.equal(f.cpu(), cpu.faces) and torch.equal(_bits(v.cpu()), _bits(cpu.vertices))
    assert target - 1 <= len(f) < len(f0) and tuple(colors.shape) == (len(v), 3) and tuple(frames.shape) == (2, 64, 64, 3)
    with pytest.raises(ValueError):
        mesh.extract_mesh(G, ws, target_faces=target, cell=0.1, **kw)
