"""pix2pix3d_amd.reproject on the device: the bytes of p3d_view_splat / p3d_view_resolve / p3d_view_difference_histogram against the CPU formulation (integer
equality, the regions library's launch counter moving by exactly one per primitive and by nothing for no frames), the accumulator without a synchronising
call, and the generator and the edit session end to end.  The shapes are the smallest at which the kernels can go wrong: one point into one pixel, sizes that
are no multiple of a work-group, pitched views off every alignment, every point on one pixel, footprints clipped at all four corners, more than one frame
with a broadcast source, a source and a target of different sizes."""
import inspect

import pytest
import torch

from views_cases import to_device_same_layout
from edit_cases import Counters, random_mask
from model_cases import build_generator
from reproject_cases import EMPTY, cameras_at, planted_points, sphere_scene, view_in_canvas
from test_edit_gpu import bench_session          # noqa: F401  (the fixtures of the edit and sketch tests, reused as they are)
from test_sketch_gpu import small_session        # noqa: F401

pytestmark = pytest.mark.gpu

ANGLES = [(0.0, 0.0), (0.1, -0.05), (-0.2, 0.1)]


def _ran(n0, launches):
    from pix2pix3d_amd import regions
    torch.cuda.synchronize()
    assert regions.launch_count() == n0 + launches, (regions.launch_count() - n0, launches)


def _splat_equal(points, cameras, size=None, radius=0, valid=None, dev_valid=None, launches=1):
    from pix2pix3d_amd import regions, reproject
    want = reproject.splat(points, cameras, size, radius, valid)
    n0 = regions.launch_count()
    got = reproject.splat(points.cuda(), cameras.cuda(), size, radius, dev_valid if dev_valid is not None else (None if valid is None else valid.cuda()))
    _ran(n0, launches)
    bad = int((got.cpu() != want).sum())
    print('points', tuple(points.shape), 'into', tuple(want.shape), 'radius', radius, 'covered', int((want != EMPTY).sum()), 'differing cells', bad)
    assert got.dtype == torch.int64 and got.is_cuda and got.is_contiguous() and bad == 0
    return want


# ---- 1. splat ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cameras():
    return cameras_at(ANGLES)


def test_splat_of_one_point_into_one_pixel_and_of_small_views(hip_lib, cameras):
    one = torch.tensor([0.01, -0.02, 0.1]).view(1, 1, 1, 3)
    want = _splat_equal(one, cameras[:1], size=(1, 1))
    assert int(want.item()) & 0xffffffff == 0 and int(want.item()) != EMPTY
    for radius in (0, 1, 2):
        _splat_equal(planted_points(1, 3, 5, seed=1) * 0.3, cameras[:1], size=(5, 3), radius=radius)


@pytest.mark.parametrize('shift', [0, 1, 2, 3])
def test_splat_with_a_pitched_valid_view_inside_a_canvas(hip_lib, cameras, shift):
    pts = planted_points(3, 67, 131, seed=2)
    valid = view_in_canvas((torch.rand(3, 67, 131, generator=torch.Generator().manual_seed(3)) < 0.7).to(torch.uint8) * 3, shift)
    dev = to_device_same_layout(valid)
    assert dev.stride() == valid.stride() and dev.stride(1) > 131
    want = _splat_equal(pts, cameras, radius=1, valid=valid, dev_valid=dev)
    assert not torch.equal(want, _splat_equal(pts, cameras, radius=1))


def test_splat_where_every_point_lands_on_one_pixel(hip_lib, cameras):
    """16384 points along the central ray, nearer with a growing index until the middle and farther after it: 64-way contention on one address in every wave;
    the winner is the smallest key."""
    k = torch.arange(16384, dtype=torch.float32)
    pts = torch.zeros(1, 128, 128, 3)
    pts[..., 2] = (0.4 - (k - 8000).abs() / 20000).view(1, 128, 128)
    pts[0, 62, 64:70] = pts[0, 62, 64]                                                  # equal keys but for the index around the nearest point (index 8000)
    want = _splat_equal(pts, cameras[:1], size=(9, 9))
    assert int((want != EMPTY).sum()) == 1 and int(want[0, 4, 4]) & 0xffffffff == 8000
    want = _splat_equal(pts, cameras[:1], size=(9, 9), radius=2)
    assert int((want != EMPTY).sum()) == 25 and bool((want[0, 2:7, 2:7] == want[0, 4, 4]).all())


def test_splat_clips_footprints_at_the_four_corners(hip_lib, cameras):
    """Radius 2 with points on the corner pixels and one, two and three pixels outside: only the in-image part of a footprint is written."""
    from pix2pix3d_amd import reproject
    cam = cameras[:1]
    z, focal, size = 2.7 - 0.2, 4.2647, 16
    pts = []
    for px in (-3.5, -2.5, -0.5, 0.5, 15.5, 16.5, 18.5, 19.5):
        for py in (-3.5, -1.5, 0.5, 15.5, 17.5, 19.5):
            u, v = px / size, py / size
            pts.append([(u - 0.5) * z / focal, -(v - 0.5) * z / focal, 0.2])             # camera y and z are world -y and -z for this camera
    pts = torch.tensor(pts).view(1, 1, len(pts), 3)
    for radius in (0, 1, 2):
        want = _splat_equal(pts, cam, size=(size, size), radius=radius)
        assert int((want != EMPTY).sum()) > 0
    assert bool((want[0, 0, 0] != EMPTY) & (want[0, 15, 15] != EMPTY) & (want[0, 0, 15] != EMPTY) & (want[0, 15, 0] != EMPTY)) and int(want[0, 8, 8]) == EMPTY
    assert reproject.GUARD == 4


def test_splat_of_three_cameras_with_a_broadcast_source_and_of_another_size(hip_lib, cameras):
    from pix2pix3d_amd import regions, reproject
    s = sphere_scene([(0.0, 0.0)], 128)
    want = _splat_equal(s['points'], cameras)                                          # [1, 128, 128, 3] seen by three cameras
    assert torch.equal(want, _splat_equal(s['points'][0], cameras))
    _splat_equal(s['points'], cameras[:1], size=(96, 160))
    _splat_equal(s['points'], cameras, size=(96, 160), radius=2)
    _splat_equal(planted_points(3, 24, 20), cameras, size=(17, 29), radius=1)          # the planted drops
    n0 = regions.launch_count()
    assert reproject.splat(s['points'][:0].cuda(), cameras[:0].cuda()).numel() == 0
    _ran(n0, 0)
    out = reproject.splat(s['points'].cuda(), cameras.cuda())                           # a second splat into a buffer that holds keys
    assert reproject.splat((s['points'] * 0.9).cuda(), cameras.cuda(), out=out) is out
    assert torch.equal(out.cpu(), reproject.splat(s['points'] * 0.9, cameras, out=want.clone()))


# ---- 2. resolve ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def resolve_case(cameras):
    """(zbuf [3, 37, 61] from 67 x 131 points, target points [3, 37, 61, 3]): shared, never modified."""
    from pix2pix3d_amd import reproject
    zbuf = reproject.splat(planted_points(3, 67, 131, seed=4), cameras, size=(37, 61))
    assert 0 < int((zbuf == EMPTY).sum()) < zbuf.numel()
    return zbuf, planted_points(3, 37, 61, seed=5)


def _resolve_equal(zbuf, source, fill, target, cameras, tolerance, dev_source=None, counts=False, index=True):
    from pix2pix3d_amd import regions, reproject
    c0 = torch.arange(5, dtype=torch.int64) * 1000 if counts else None
    want = reproject.resolve(zbuf, source, fill, target, cameras, tolerance, counts=None if c0 is None else c0.clone(), return_index=index)
    dc = None if c0 is None else c0.cuda()
    n0 = regions.launch_count()
    got = reproject.resolve(zbuf.cuda(), source.cuda() if dev_source is None else dev_source, fill, None if target is None else target.cuda(),
                            None if cameras is None else cameras.cuda(), tolerance, counts=dc, return_index=index)
    _ran(n0, 1 if zbuf.shape[0] else 0)
    for g, w, name in zip(got, want, ('warped', 'status', 'index')):
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape) and torch.equal(g.cpu(), w), name
    if counts:
        assert torch.equal(dc.cpu(), c0 + torch.bincount(want[1].reshape(-1).long(), minlength=5))
    return want


@pytest.mark.parametrize('channels', [1, 3, 4])
def test_resolve_of_pitched_sources_off_every_alignment(hip_lib, cameras, resolve_case, channels):
    zbuf, target = resolve_case
    source = torch.randint(0, 256, [3, 67, 131, channels], generator=torch.Generator().manual_seed(6), dtype=torch.uint8)
    fill = [200, 201, 202, 203][:channels]
    want = _resolve_equal(zbuf, source, fill, target, cameras, 3000, counts=True)
    assert len(set(want[1].unique().tolist())) >= 3
    _resolve_equal(zbuf, source, fill, None, None, None, counts=True, index=False)
    _resolve_equal(zbuf, source[:1], fill, target, cameras, 0)                          # a broadcast source
    for shift in (0, 1, 2, 3):
        view = view_in_canvas(source, shift)
        _resolve_equal(zbuf, view, fill, None, None, None, dev_source=to_device_same_layout(view), index=False)
    if channels == 1:
        _resolve_equal(zbuf, source[..., 0], 7, None, None, None)                      # [F, h, w]
    from pix2pix3d_amd import reproject
    want, _ = reproject.resolve(zbuf, source, fill)
    for shift in (0, 1, 2, 3):                                                        # a pitched destination inside a canvas of 77s: the bytes around it stay
        canvas = view_in_canvas(torch.full([3, 37, 61, channels], 77, dtype=torch.uint8), shift)
        dev = to_device_same_layout(canvas)
        got, _ = reproject.resolve(zbuf.cuda(), source.cuda(), fill, out=dev)
        host = torch.as_strided(dev, [dev.untyped_storage().nbytes()], [1], 0).cpu()
        assert got is dev and torch.equal(dev.cpu(), want)
        assert int((host != 77).sum()) == int((want != 77).sum()), shift


def test_resolve_of_an_empty_buffer_and_of_one_covered_pixel(hip_lib, cameras, resolve_case):
    from pix2pix3d_amd import regions, reproject
    _, target = resolve_case
    source = torch.randint(0, 256, [3, 67, 131, 3], generator=torch.Generator().manual_seed(7), dtype=torch.uint8)
    zbuf = torch.full([3, 37, 61], EMPTY, dtype=torch.int64)
    want = _resolve_equal(zbuf, source, [1, 2, 3], target, cameras, 5, counts=True)
    assert bool((want[1] == 0).all()) and bool((want[2] == -1).all()) and bool((want[0] == torch.tensor([1, 2, 3], dtype=torch.uint8)).all())
    zbuf[1, 36, 60] = (70000 << 32) + 67 * 131 - 1                                      # the last source pixel on the last target pixel
    zbuf[2, 0, 0] = (5 << 32) + 67 * 131                                                # an index past the source: a hole, never read
    want = _resolve_equal(zbuf, source, [1, 2, 3], None, None, None, counts=True)
    assert int((want[1] == 1).sum()) == 1 and torch.equal(want[0][1, 36, 60], source[1, 66, 130]) and int(want[2][1, 36, 60]) == 67 * 131 - 1
    n0 = regions.launch_count()
    got = reproject.resolve(zbuf[:0].cuda(), source[:0].cuda())
    _ran(n0, 0)
    assert got[0].numel() == 0 and got[1].numel() == 0


def test_resolve_counts_accumulate_over_two_calls(hip_lib, cameras, resolve_case):
    from pix2pix3d_amd import reproject
    zbuf, target = resolve_case
    source = torch.zeros([3, 67, 131], dtype=torch.uint8)
    counts = torch.zeros(5, dtype=torch.int64, device='cuda')
    for _ in range(2):
        reproject.resolve(zbuf.cuda(), source.cuda(), 0, target.cuda(), cameras.cuda(), 3000, counts=counts)
    _, status = reproject.resolve(zbuf, source, 0, target, cameras, 3000)
    assert torch.equal(counts.cpu(), 2 * torch.bincount(status.reshape(-1).long(), minlength=5)) and int(counts.sum()) == 2 * zbuf.numel()


# ---- 3. difference histogram -------------------------------------------------------------------------------------------------------------
def _differences_equal(a, b, where=None, match=1, dev=None):
    from pix2pix3d_amd import regions, reproject
    want = reproject.difference_histogram(a, b, where, match)
    da, db, dw = dev if dev is not None else (a.cuda(), b.cuda(), None if where is None else where.cuda())
    n0 = regions.launch_count()
    got = reproject.difference_histogram(da, db, dw, match)
    _ran(n0, 1)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want), (got.cpu() - want).nonzero().tolist()
    return want


def test_difference_histogram_equals_the_cpu_formulation(hip_lib):
    g = torch.Generator().manual_seed(8)
    a = torch.randint(0, 256, [3, 67, 131, 3], generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, [3, 67, 131, 3], generator=g, dtype=torch.uint8)
    where = torch.randint(0, 3, [3, 67, 131], generator=g, dtype=torch.uint8)
    want = _differences_equal(a, a.clone())
    assert int(want[0]) == a.numel() and int(want[1:].sum()) == 0                      # identical frames: everything in bin 0
    want = _differences_equal(torch.zeros_like(a), torch.full_like(a, 255))
    assert int(want[255]) == a.numel()                                                 # 255 apart
    _differences_equal(a, b)
    _differences_equal(a, b, where, 1)
    assert int(_differences_equal(a, b, torch.ones_like(where), 1).sum()) == a.numel()
    assert int(_differences_equal(a, b, where, 7).sum()) == 0
    _differences_equal(a[:1, :1, :1], b[:1, :1, :1], where[:1, :1, :1], 0)             # 1 x 1
    _differences_equal(a[..., 0].contiguous(), b[..., 0].contiguous(), where)                                    # [F, H, W]
    _differences_equal(torch.cat([a, a[..., :1]], dim=-1), torch.cat([b, b[..., :1]], dim=-1), where, 2)      # four channels
    for shift in (0, 1, 2, 3):
        va, vb, vw = view_in_canvas(a, shift), view_in_canvas(b, (shift + 1) % 4), view_in_canvas(where, shift)
        _differences_equal(va, vb, vw, 1, dev=(to_device_same_layout(va), to_device_same_layout(vb), to_device_same_layout(vw)))


# ---- 4. the accumulator --------------------------------------------------------------------------------------------------------------------
def test_add_issues_no_synchronising_call(hip_lib):
    from pix2pix3d_amd import regions, reproject
    s = sphere_scene([(0.0, 0.0), (0.1, -0.05), (0.35, 0.0)], 64)
    dev = {k: v.cuda() for k, v in s.items()}
    pairs, tol = [(0, 1), (1, 0), (0, 2), (2, 2)], round(0.02 * 65536)
    regions.regions_lib()
    reproject.points(dev['depth'], dev['cameras'])                                       # (the ray sampler's library is loaded before the mode is set)
    total = reproject.Consistency(8, 'cuda')
    plain = reproject.Consistency(None, 'cuda')
    torch.cuda.synchronize()
    n0 = regions.launch_count()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        total.add(dev['labels'], dev['images'], dev['depth'], dev['cameras'], pairs, tol)
        total.add(dev['labels'], dev['images'], dev['depth'], dev['cameras'], pairs[:1], tol, radius=1)
        plain.add(None, dev['images'], dev['depth'], dev['cameras'], pairs, tol)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    _ran(n0, 2 * reproject.COUNT_LAUNCHES[True] + reproject.COUNT_LAUNCHES[False])
    for fn in (reproject.Consistency.add, reproject.consistency_counts, reproject.splat, reproject.resolve, reproject.difference_histogram, reproject.points):
        source = inspect.getsource(fn)
        assert not any(word in source for word in ('.item(', '.cpu(', '.tolist(', '.numpy(', 'synchronize', 'bool(')), fn.__name__
    # the device's points differ from the CPU's in the last bit (another ray sampler): the counters are compared on the device's own points
    pts = reproject.points(dev['depth'], dev['cameras']).cpu()
    host, host_plain = reproject.Consistency(8, 'cpu'), reproject.Consistency(None, 'cpu')
    for which, radius in ((pairs, 0), (pairs[:1], 1)):
        src, dst = [i for i, _ in which], [j for _, j in which]
        zbuf = reproject.splat(pts[src], s['cameras'][dst], radius=radius)
        labels, status = reproject.resolve(zbuf, s['labels'][src], 0, pts[dst], s['cameras'][dst], tol, counts=host.status)
        images, _ = reproject.resolve(zbuf, s['images'][src])
        from pix2pix3d_amd import evaluate
        evaluate.confusion(s['labels'][dst], labels, 8, valid=status == 1, out=host.confusion)
        reproject.difference_histogram(s['images'][dst], images, status, 1, out=host.differences)
        if radius == 0:
            host_plain.status += torch.bincount(status.reshape(-1).long(), minlength=5)
            reproject.difference_histogram(s['images'][dst], images, status, 1, out=host_plain.differences)
    for got, want in ((total, host), (plain, host_plain)):
        assert torch.equal(got.status.cpu(), want.status) and torch.equal(got.confusion.cpu(), want.confusion) and torch.equal(got.differences.cpu(), want.differences)
    r = total.result()
    print({k: r[k] for k in ('coverage', 'consistent', 'behind', 'in_front', 'mad', 'psnr')}, 'accuracy', r['labels']['accuracy'])
    assert r['pairs'] == 5 and r['coverage'] > 0.5 and r['pixels'] == 5 * 64 * 64 and plain.result()['labels'] is None


# ---- 5. the generator and the session ------------------------------------------------------------------------------------------------------
def test_video_consistency_of_identity_pairs(hip_lib):
    """Every frame warped into its own camera: coverage 1, every pixel consistent at tolerance 0, a diagonal confusion matrix, differences in bin 0 only —
    and ONE backbone pass for the whole path."""
    from pix2pix3d_amd import reproject
    from pix2pix3d_amd import edit
    G = build_generator('seg2cat', 'cuda', depth=(64, 64))                             # the generator of ``bench_session``: built once for the suite
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(1)).cuda()
    fwd = edit.forward_label(G).cuda()
    ws = G.mapping(z, fwd, {'mask': random_mask(1, 512, 512, 6, seed=54)[None].cuda(), 'pose': fwd}, truncation_psi=0.75)
    c = Counters(G)
    try:
        r = reproject.video_consistency(G, ws, 'seg2cat', n_frames=3, stride=0, jitter='frozen', tolerance=0, neural_rendering_resolution=32)
        assert c.take()[2] == 1
        turned = reproject.video_consistency(G, ws, 'seg2cat', n_frames=3, stride=1, jitter='frozen', neural_rendering_resolution=32)
    finally:
        c.remove()
    print({k: r[k] for k in ('coverage', 'consistent', 'mad')}, 'stride 1:', {k: turned[k] for k in ('coverage', 'consistent', 'behind', 'in_front', 'mad', 'tolerance')})
    assert r['pixels'] == 3 * 32 * 32 and r['coverage'] == 1.0 and r['consistent'] == 1.0 and r['pairs'] == 3 and r['tolerance'] == 0 and r['stride'] == 0
    matrix = r['labels']['matrix']
    assert int(matrix.sum()) == 3 * 32 * 32 and torch.equal(matrix, torch.diag(matrix.diagonal()))
    assert int(r['differences'][0]) == 3 * 32 * 32 * 3 and int(r['differences'][1:].sum()) == 0 and r['psnr'] == float('inf')
    assert turned['pairs'] == 2 and turned['pixels'] == 2 * 32 * 32 and turned['tolerance'] == reproject.default_tolerance(G)


def test_edit_session_consistency(bench_session):
    from pix2pix3d_amd import reproject
    G, s, u, base, pose = bench_session
    s.render()
    c = Counters(G)
    try:
        got = s.consistency(yaw=0.1)
        torch.cuda.synchronize()
        assert c.take() == (0, 0, 0)                                                    # neither the Encoder nor the backbone
    finally:
        c.remove()
    v = got['views']
    first = reproject.raw_frames(s.render(return_float=True)['float'])
    assert torch.equal(v['labels'][0], first['labels'][0]) and torch.equal(v['images'][0], first['images'][0]) and torch.equal(v['depth'][0], first['depth'][0])
    assert torch.equal(v['cameras'][:1], s.camera) and not torch.equal(v['cameras'][1], v['cameras'][0]) and tuple(v['labels'].shape) == (2, 128, 128)
    want = reproject.consistency_counts(v['labels'], v['images'], v['depth'], v['cameras'], [(0, 1)], 6, got['tolerance']).result()
    print({k: got[k] for k in ('coverage', 'consistent', 'behind', 'in_front', 'mad', 'psnr', 'tolerance')}, 'accuracy', got['labels']['accuracy'])
    assert torch.equal(got['status_counts'], want['status_counts']) and torch.equal(got['differences'], want['differences'])
    assert torch.equal(got['labels']['matrix'], want['labels']['matrix']) and got['pixels'] == 128 * 128 and got['n_labels'] == 6
    assert got['tolerance'] == reproject.default_tolerance(G)


def test_sketch_session_consistency(small_session):
    """An edge generator has no label maps: the grey map travels as the images' fourth channel and the confusion counter stays empty."""
    from pix2pix3d_amd import reproject
    G, s, u = small_session
    s.render()
    c = Counters(G)
    try:
        got = s.consistency(yaw=0.1, pitch=-0.05)
        torch.cuda.synchronize()
        assert c.take() == (0, 0, 0)
    finally:
        c.remove()
    v = got['views']
    assert v['labels'] is None and got['labels'] is None and got['n_labels'] is None and v['images'].shape[0] == 2 and v['images'].shape[-1] == 4
    want = reproject.consistency_counts(None, v['images'], v['depth'], v['cameras'], [(0, 1)], None, got['tolerance']).result()
    print({k: got[k] for k in ('coverage', 'consistent', 'behind', 'in_front', 'mad', 'psnr', 'tolerance')})
    assert torch.equal(got['status_counts'], want['status_counts']) and torch.equal(got['differences'], want['differences'])
    assert got['pixels'] == v['depth'][0].numel() and int(got['differences'].sum()) == 4 * int(got['status_counts'][1])
