"""pix2pix3d_amd.evaluate on the device: the counts of p3d_label_confusion / p3d_label_boundary / p3d_label_distance_histogram against the CPU formulation
(integer equality, the regions library's launch counter moving by exactly the documented count), and the sessions, the accumulator and the generator loop at
bench size.  The shapes are the smallest at which the kernels can go wrong: pitched views off every alignment (the 16-byte loads' head and tail, the byte
route, the frame pitch), rows of one and of 4096 pixels, one key in every lane, no two equal neighbours."""
import inspect

import pytest
import torch

from views_cases import to_device_same_layout
from edit_cases import random_mask, Counters
from regions_cases import spiral, checkerboard
from sketch_cases import crossing_lines
from test_edit_gpu import bench_session          # noqa: F401  (the fixtures of the edit and sketch tests, reused as they are)
from test_sketch_gpu import small_session        # noqa: F401

pytestmark = pytest.mark.gpu


def _view_in_canvas(maps, shift):
    """``maps`` [N, H, W] as a device view with row pitch W + 6, frame pitch (H + 2) (W + 6) and a pointer ``shift`` bytes off, inside a canvas of 77s."""
    n, h, w = maps.shape
    store = torch.full([n * (h + 2) * (w + 6) + 8], 77, dtype=torch.uint8)
    view = store[shift:shift + n * (h + 2) * (w + 6)].view(n, h + 2, w + 6)[:, 1:1 + h, 2:2 + w]
    view.copy_(maps)
    dev = to_device_same_layout(view)
    assert dev.stride() == ((h + 2) * (w + 6), w + 6, 1) and torch.equal(dev.cpu(), maps)
    return dev


def _ran(n0, launches):
    from pix2pix3d_amd import regions
    torch.cuda.synchronize()
    assert regions.launch_count() == n0 + launches, (regions.launch_count() - n0, launches)


def _confusion_equal(truth, pred, n_labels, valid=None, dev=None, launches=1):
    from pix2pix3d_amd import evaluate, regions
    want = evaluate.confusion(truth, pred, n_labels, valid)
    t, p, v = dev if dev is not None else (truth.cuda(), pred.cuda(), None if valid is None else valid.cuda())
    n0 = regions.launch_count()
    got = evaluate.confusion(t, p, n_labels, v)
    _ran(n0, launches)
    bad = int((got.cpu() != want).sum())
    print(tuple(truth.shape), 'labels', n_labels, 'pixels', int(want.sum()), 'left out', int(want[-1]), 'differing cells', bad)
    assert got.dtype == torch.int64 and got.is_cuda and int(want.sum()) == truth.numel() and bad == 0
    return want


# ---- 1. confusion ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pitched_case():
    """(truth, pred, valid) [3, 67, 131], 19 labels: shared, never modified."""
    g = torch.Generator().manual_seed(3)
    return random_mask(3, 67, 131, 19, seed=1), random_mask(3, 67, 131, 19, seed=2), (torch.rand(3, 67, 131, generator=g) < 0.8).to(torch.uint8) * 9


@pytest.mark.parametrize('shifts', [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 2, 3), (3, 3, 1), (2, 1, None), (3, 3, None)])
def test_confusion_of_pitched_views_off_every_alignment(hip_lib, pitched_case, shifts):
    """Equal shifts: every row takes the 16-byte loads behind a scalar head (a row pitch of 137 moves the head from row to row); unequal ones: the byte route."""
    truth, pred, valid = pitched_case
    valid = None if shifts[2] is None else valid
    dev = (_view_in_canvas(truth, shifts[0]), _view_in_canvas(pred, shifts[1]), None if valid is None else _view_in_canvas(valid, shifts[2]))
    want = _confusion_equal(truth, pred, 19, valid, dev=dev)
    assert (int(want[-1]) > 0) == (valid is not None)


@pytest.mark.parametrize('shape', [(1, 64, 4096), (1, 4096, 3), (5, 1, 1), (2, 3, 4097 // 17)])
def test_confusion_of_long_rows_and_short_rows(hip_lib, shape):
    truth, pred = random_mask(shape[0], shape[1], shape[2], 6, seed=4), random_mask(shape[0], shape[1], shape[2], 6, seed=5)
    _confusion_equal(truth, pred, 6)                                                   # everything abuts: ONE row of N H W pixels
    views = []
    if shape[1] > 1:
        views.append((truth[:, 1:, :], pred[:, :-1, :]))                               # frames that do not abut: a row per frame
    if shape[2] > 32:
        views.append((truth[:, :, 1:-2], pred[:, :, 3:]))                              # rows that do not abut, operands 2 bytes apart in alignment: the byte route
        views.append((truth[:, :, 16:], pred[:, :, :-16]))                             # rows that do not abut, one alignment: the 16-byte loads
    for t, p in views:
        _confusion_equal(t, p, 6, dev=(to_device_same_layout(t), to_device_same_layout(p), None))


def test_confusion_where_every_lane_holds_one_key_and_where_no_two_neighbours_agree(hip_lib):
    single = torch.full([2, 256, 256], 2, dtype=torch.uint8)
    want = _confusion_equal(single, single.clone(), 6)
    assert int(want[2 * 6 + 2]) == 2 * 256 * 256
    other = single.clone()
    other[1, 100:, :] = 5                                                            # whole waves of one key, two keys in the work-group's tile at the seam
    other[0, 7, 9] = 0
    _confusion_equal(single, other, 6)
    board = checkerboard(67, 131)
    want = _confusion_equal(board, checkerboard(67, 131, 4, 1), 6)
    assert int(want[1 * 6 + 4]) + int(want[4 * 6 + 1]) == 67 * 131
    _confusion_equal(board, board.clone(), 6)


@pytest.mark.parametrize('n_labels', [1, 6, 32])
def test_confusion_with_labels_out_of_range_and_a_valid_mask(hip_lib, n_labels):
    truth, pred = random_mask(2, 67, 131, 40, seed=6), random_mask(2, 67, 131, 40, seed=7)
    truth[0, :3] = 255
    valid = torch.rand(2, 67, 131, generator=torch.Generator().manual_seed(8)) < 0.6
    want = _confusion_equal(truth, pred, n_labels)
    assert int(want[-1]) > 0
    _confusion_equal(truth, pred, n_labels, valid)
    _confusion_equal(truth[0], pred[0], n_labels, valid[0])                              # [H, W]


def test_confusion_accumulates_and_no_frames_launch_nothing(hip_lib):
    from pix2pix3d_amd import evaluate, regions
    truth, pred = random_mask(3, 67, 131, 6, seed=9), random_mask(3, 67, 131, 6, seed=10)
    want = evaluate.confusion(truth, pred, 6)
    out = torch.zeros(37, dtype=torch.int64, device='cuda')
    n0 = regions.launch_count()
    assert evaluate.confusion(truth[:2].cuda(), pred[:2].cuda(), 6, out=out) is out
    evaluate.confusion(truth[2].cuda(), pred[2].cuda(), 6, out=out)
    _ran(n0, 2)
    assert torch.equal(out.cpu(), want)
    evaluate.confusion(truth[:0].cuda(), pred[:0].cuda(), 6, out=out)
    _ran(n0, 2)
    assert torch.equal(out.cpu(), want)


# ---- 2. boundary and distance histogram --------------------------------------------------------------------------------------------------
def _map_cases():
    return {'spiral 64': (spiral(64), torch.rot90(spiral(64), 1, [0, 1]).contiguous()), 'blobs 512': (random_mask(1, 512, 512, 6, seed=11)[0], random_mask(1, 512, 512, 6, seed=12)[0]),
            '1x1': (torch.full([1, 1], 3, dtype=torch.uint8), torch.full([1, 1], 3, dtype=torch.uint8)),
            '1x300': (random_mask(1, 1, 300, 4, seed=13)[0], random_mask(1, 1, 300, 4, seed=14)[0]), 'checkerboard 67x131': (checkerboard(67, 131), checkerboard(67, 131, 4, 1))}


@pytest.fixture(scope='module')
def map_refs():
    """name -> (a, b, CPU boundary of a, CPU boundary of b, CPU nearest boundary pixel of a): computed once, never modified."""
    from pix2pix3d_amd import evaluate, regions
    refs = {}
    for name, (a, b) in _map_cases().items():
        ba, bb = evaluate.boundary(a), evaluate.boundary(b)
        refs[name] = (a, b, ba, bb, regions.nearest(ba, evaluate.CLASS_AGNOSTIC))
    return refs


@pytest.mark.parametrize('name', sorted(_map_cases()))
def test_boundary_equals_the_cpu_formulation(hip_lib, map_refs, name):
    from pix2pix3d_amd import evaluate, regions
    a, b, ba, bb, _ = map_refs[name]
    for m, want in ((a, ba), (b, bb)):
        n0 = regions.launch_count()
        got = evaluate.boundary(m.cuda())
        _ran(n0, 1)
        bad = int((got.cpu() != want).sum())
        print(name, 'boundary pixels', int((want != 255).sum()), 'differing bytes', bad)
        assert got.dtype == torch.uint8 and got.is_contiguous() and bad == 0


def test_boundary_of_pitched_misaligned_views(hip_lib):
    from pix2pix3d_amd import evaluate
    mask = random_mask(1, 67, 131, 19, seed=15)
    want = evaluate.boundary(mask[0])
    for shift in (0, 1, 2, 3):
        assert torch.equal(evaluate.boundary(_view_in_canvas(mask, shift)[0]).cpu(), want), shift


@pytest.mark.parametrize('name', sorted(_map_cases()))
def test_distance_histogram_equals_the_cpu_formulation(hip_lib, map_refs, name):
    """bins 1 and 4096 are the limits; the empty site set counts nothing; a nearest map of -1 puts every pixel of the set into the last slot."""
    from pix2pix3d_amd import evaluate, regions
    a, b, ba, bb, near = map_refs[name]
    bb_dev, near_dev = bb.cuda(), near.cuda()
    nothing = torch.full_like(near, -1)
    for sites, bins, q in ((evaluate.CLASS_AGNOSTIC, 65, near), (evaluate.CLASS_AGNOSTIC, 1, near), (evaluate.CLASS_AGNOSTIC, 4096, near), ((3, 4), 10, near),
                           ((), 65, near), (evaluate.CLASS_AGNOSTIC, 65, nothing)):
        want = evaluate.distance_histogram(bb, sites, q, bins)
        n0 = regions.launch_count()
        got = evaluate.distance_histogram(bb_dev, sites, near_dev if q is near else nothing.cuda(), bins)
        _ran(n0, 1)
        bad = int((got.cpu() != want).sum())
        print(name, 'sites', len(sites), 'bins', bins, 'pixels', int(want.sum()), 'saturated', int(want[-2]), 'no site', int(want[-1]), 'differing slots', bad)
        assert got.dtype == torch.int64 and bad == 0
        assert (len(sites) > 0) or int(want.sum()) == 0
        assert q is near or int(want[-1]) == int(want.sum()) == int((bb != 255).sum())
    out = torch.zeros(67, dtype=torch.int64, device='cuda')                                # two accumulating calls, from a pitched view
    view = _view_in_canvas(bb[None], 3)[0]
    evaluate.distance_histogram(view, evaluate.CLASS_AGNOSTIC, near_dev, 65, out=out)
    evaluate.distance_histogram(view, evaluate.CLASS_AGNOSTIC, near_dev, 65, out=out)
    assert torch.equal(out.cpu(), 2 * evaluate.distance_histogram(bb, evaluate.CLASS_AGNOSTIC, near, 65))


def test_boundary_counts_per_class_and_ink_counts(hip_lib):
    from pix2pix3d_amd import evaluate, regions
    truth, pred = random_mask(1, 128, 128, 6, seed=16)[0], random_mask(1, 128, 128, 6, seed=17)[0]
    pred = torch.where(torch.rand(128, 128, generator=torch.Generator().manual_seed(18)) < 0.7, truth, pred)
    n0 = regions.launch_count()
    got = evaluate.boundary_counts(truth.cuda(), pred.cuda(), n_labels=6, per_class=True)
    _ran(n0, 2 + 6 * 6)
    assert tuple(got.shape) == (6, 2, 67) and torch.equal(got.cpu(), evaluate.boundary_counts(truth, pred, n_labels=6, per_class=True))
    n0 = regions.launch_count()
    both = evaluate.boundary_counts(torch.stack([truth, pred]).cuda(), torch.stack([pred, pred]).cuda())
    _ran(n0, 2 * evaluate.BOUNDARY_LAUNCHES)
    assert torch.equal(both.cpu(), evaluate.boundary_counts(truth, pred) + evaluate.boundary_counts(pred, pred))
    ink_a, ink_b = crossing_lines(128, 128, step=16), torch.roll(crossing_lines(128, 128, step=16), (2, 1), (0, 1))
    n0 = regions.launch_count()
    ink = evaluate.ink_counts(ink_a.cuda(), ink_b.cuda())
    _ran(n0, evaluate.INK_LAUNCHES)
    assert torch.equal(ink.cpu(), evaluate.ink_counts(ink_a, ink_b)) and int(ink.sum()) > 0
    assert evaluate.ink_agreement(ink_a.cuda(), ink_b.cuda(), tolerance=3) == evaluate.ink_agreement(ink_a, ink_b, tolerance=3)


# ---- 3. the accumulator, the sessions and the generator loop ---------------------------------------------------------------------------------
def _same_result(a, b):
    for key in ('matrix', 'boundary_counts', 'ink_counts'):
        assert torch.equal(a[key], b[key]), key
    for key in ('pixels', 'left_out', 'frames', 'ink_frames', 'n_labels'):
        assert a[key] == b[key], key
    for key in ('accuracy', 'miou', 'fw_iou'):
        assert a[key] == b[key] or (a[key] != a[key] and b[key] != b[key]), key
    assert repr(a['boundary']) == repr(b['boundary']) and repr(a['ink']) == repr(b['ink']) and repr(a['iou']) == repr(b['iou'])


def test_add_issues_no_synchronising_call(hip_lib):
    """``add`` / ``add_ink`` under torch's sync debug mode 'error' (any synchronising torch call raises), their launches on the regions counter, and no
    host read in their source."""
    from pix2pix3d_amd import evaluate, regions
    truth, pred = random_mask(2, 128, 128, 6, seed=19), random_mask(2, 128, 128, 6, seed=20)
    ink = crossing_lines(128, 128, step=16)
    t, p, a, b = truth.cuda(), pred.cuda(), ink.cuda(), torch.roll(ink, 1, 0).cuda()
    regions.regions_lib()
    total = evaluate.Agreement(6, 'cuda')
    torch.cuda.synchronize()
    n0 = regions.launch_count()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        total.add(t, p)
        total.add(t[0], p[0], boundary=False)
        total.add_ink(a, b)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    _ran(n0, 1 + 2 * evaluate.BOUNDARY_LAUNCHES + 1 + evaluate.INK_LAUNCHES)
    for fn in (evaluate.Agreement.add, evaluate.Agreement.add_ink, evaluate.confusion, evaluate.boundary_counts, evaluate.ink_counts, evaluate._both_ways,
               evaluate.distance_histogram, evaluate.boundary):
        source = inspect.getsource(fn)
        assert not any(word in source for word in ('.item(', '.cpu(', '.tolist(', '.numpy(', 'synchronize', 'int(out', 'bool(')), fn.__name__
    host = evaluate.Agreement(6, 'cpu')
    host.add(truth, pred); host.add(truth[0], pred[0], boundary=False); host.add_ink(ink, torch.roll(ink, 1, 0))
    _same_result(total.result(), host.result())


def test_edit_session_agreement(bench_session):
    from pix2pix3d_amd import evaluate, regions
    G, s, u, base, pose = bench_session
    c = Counters(G)
    try:
        got = s.agreement()
        torch.cuda.synchronize()
        assert c.take() == (1, 1, 1)
        mask, label = s.mask.cpu(), s.render()['label_index'].cpu()
        host = evaluate.Agreement(6, 'cpu')
        host.add(mask, label)
        want = host.result()
        print('agreement at bench size', {k: got[k] for k in ('accuracy', 'miou')}, got['boundary'])
        _same_result(got, want)
        assert got['n_labels'] == 6 == int(G.semantic_channels) and got['pixels'] == 512 * 512 and got['frames'] == 1
        n0 = regions.launch_count()
        again = s.agreement()
        assert regions.launch_count() == n0 and c.take() == (0, 0, 0)             # kept with the frame
        _same_result(again, want)
        assert s.agreement(tolerance=4)['boundary']['precision'] >= got['boundary']['precision'] and regions.launch_count() == n0
        s.set_camera(yaw=40, pitch=52)
        turned = s.agreement()
        torch.cuda.synchronize()
        assert c.take() == (0, 0, 0) and regions.launch_count() == n0 + 1 + evaluate.BOUNDARY_LAUNCHES      # a camera move: neither Encoder nor backbone
        host = evaluate.Agreement(6, 'cpu')
        host.add(mask, s.render()['label_index'].cpu())
        _same_result(turned, host.result())
        assert not torch.equal(turned['matrix'], got['matrix'])
    finally:
        c.remove()


def test_sketch_session_agreement(small_session):
    from pix2pix3d_amd import evaluate, regions, sketch
    G, s, u = small_session
    with pytest.raises(ValueError):
        s.agreement()                                                           # the fixture's canvas is 300 x 260, the frame 128 x 128
    s.load(crossing_lines(128, 128, step=16), s.camera[0])
    c = Counters(G)
    try:
        got = s.agreement()
        torch.cuda.synchronize()
        assert c.take()[2] == 1
        traced = sketch.trace(255 - s.render()['label'].cpu())
        host = evaluate.Agreement(1, 'cpu')
        host.add_ink(s.canvas.cpu(), traced)
        _same_result(got, host.result())
        assert got['ink_frames'] == 1 and got['ink']['truth_pixels'] == int((s.canvas >= 128).sum())
        n0 = regions.launch_count()
        _same_result(s.agreement(), host.result())
        assert regions.launch_count() == n0 and c.take() == (0, 0, 0)
        s.set_camera(yaw=35, pitch=55)
        turned = s.agreement()
        torch.cuda.synchronize()
        assert c.take() == (0, 0, 0) and regions.launch_count() == n0 + evaluate.INK_LAUNCHES
        host = evaluate.Agreement(1, 'cpu')
        host.add_ink(s.canvas.cpu(), sketch.trace(255 - s.render()['label'].cpu()))
        _same_result(turned, host.result())
    finally:
        c.remove()


def test_evaluate_generator_equals_the_sum_over_its_items(bench_session):
    from pix2pix3d_amd import evaluate
    G, s, u, base, pose = bench_session
    items = [(base, pose), (random_mask(1, 512, 512, 6, seed=53)[0], pose)]
    got = evaluate.evaluate_generator(G, items, 'seg2cat', seed=7, truncation_psi=0.75, jitter=u)
    total = evaluate.Agreement(6, 'cuda')
    for mask, item_pose in items:
        s.load(mask, item_pose)
        total.add(s.mask, s.render()['label_index'])
    want = total.result()
    print('two items', {k: got[k] for k in ('accuracy', 'miou', 'fw_iou')}, got['boundary'])
    _same_result(got, want)
    assert got['frames'] == 2 and got['pixels'] == 2 * 512 * 512
    two = evaluate.evaluate_generator(G, items[:1], 'seg2cat', seed=7, truncation_psi=0.75, jitter=u, views_per_item=2)
    assert two['frames'] == 2 and two['pixels'] == 2 * 512 * 512
    with pytest.raises(ValueError):
        evaluate.evaluate_generator(G, [(base[:256, :256].contiguous(), pose)], 'seg2cat', jitter=u)
