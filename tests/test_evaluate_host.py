"""pix2pix3d_amd.evaluate without a GPU: the torch formulations (the definition of every count) against first principles — ``np.add.at``, four shifted copies,
a brute-force nearest site, the textbook formulas —, the conventions of the metrics, every ValueError, and the binding of the three entry points that
joined libp3d_regions.so.  Every comparison of counts is integer equality."""
import ctypes
import math

import numpy as np
import pytest
import torch

from edit_cases import random_mask
from regions_cases import checkerboard, brute_nearest
from evaluate_cases import oracle_confusion, oracle_boundary, oracle_histogram, oracle_boundary_counts, textbook_metrics, textbook_f


def _maps():
    """name -> (truth, pred, n_labels): shared, never modified."""
    single = torch.full([40, 50], 2, dtype=torch.uint8)
    return {'blobs 6': (random_mask(1, 67, 131, 6, seed=1)[0], random_mask(1, 67, 131, 6, seed=2)[0], 6),
            'blobs 19': (random_mask(1, 67, 131, 19, seed=3)[0], random_mask(1, 67, 131, 19, seed=4)[0], 19),
            'checkerboard': (checkerboard(23, 30), checkerboard(23, 30, 4, 1), 6),
            'single label': (single, single.clone(), 6),
            '1x1': (torch.full([1, 1], 3, dtype=torch.uint8), torch.full([1, 1], 1, dtype=torch.uint8), 6),
            '1x300': (random_mask(1, 1, 300, 4, seed=5)[0], random_mask(1, 1, 300, 4, seed=6)[0], 4),
            '300x1': (random_mask(1, 300, 1, 4, seed=7)[0], random_mask(1, 300, 1, 4, seed=8)[0], 4)}


NAMES = sorted(_maps())


# ---- 1. the primitives against the oracles ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_confusion_equals_add_at_and_its_rows_the_truth_histogram(name):
    from pix2pix3d_amd import evaluate
    truth, pred, n = _maps()[name]
    counts = evaluate.confusion(truth, pred, n)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (n * n + 1,)
    assert np.array_equal(counts.numpy(), oracle_confusion(truth.numpy(), pred.numpy(), n))
    assert np.array_equal(counts[:-1].view(n, n).sum(dim=1).numpy(), np.bincount(truth.numpy().ravel(), minlength=n)) and int(counts[-1]) == 0
    assert np.array_equal(counts[:-1].view(n, n).sum(dim=0).numpy(), np.bincount(pred.numpy().ravel(), minlength=n))


def test_out_of_range_labels_and_valid_land_in_the_last_slot():
    from pix2pix3d_amd import evaluate
    truth, pred = random_mask(1, 67, 131, 19, seed=9)[0], random_mask(1, 67, 131, 19, seed=10)[0]
    valid = torch.from_numpy(np.random.RandomState(0).rand(67, 131) < 0.7)
    for n in (1, 6, 19, 32):
        for v in (None, valid, valid.to(torch.uint8) * 200):
            counts = evaluate.confusion(truth, pred, n, valid=v)
            want = oracle_confusion(truth.numpy(), pred.numpy(), n, None if v is None else v.numpy())
            assert np.array_equal(counts.numpy(), want), (n, v is None)
            assert int(counts.sum()) == 67 * 131 and (n >= 19 and v is None) == (int(counts[-1]) == 0)
    marked = truth.clone()
    marked[:5] = 255
    assert int(evaluate.confusion(marked, pred, 19)[-1]) == 5 * 131                       # 255 as "ignore" in the truth


def test_batches_pitched_views_and_two_adds():
    from pix2pix3d_amd import evaluate
    truth, pred = random_mask(3, 37, 53, 6, seed=11), random_mask(3, 37, 53, 6, seed=12)
    whole = evaluate.confusion(truth, pred, 6)
    assert np.array_equal(whole.numpy(), oracle_confusion(truth.numpy(), pred.numpy(), 6))
    out = torch.zeros(37, dtype=torch.int64)
    assert evaluate.confusion(truth[:1], pred[:1], 6, out=out) is out
    evaluate.confusion(truth[1:], pred[1:], 6, out=out)                               # two adds = one add of the concatenation
    assert torch.equal(out, whole)
    view_t, view_p = truth[:, 3:30, 5:41], pred[:, 3:30, 5:41]                             # pitched views, not contiguous
    assert not view_t.is_contiguous()
    assert np.array_equal(evaluate.confusion(view_t, view_p, 6).numpy(), oracle_confusion(view_t.numpy(), view_p.numpy(), 6))
    assert int(evaluate.confusion(truth[:0], pred[:0], 6).sum()) == 0                      # no frames
    total = evaluate.Agreement(6, 'cpu')
    total.add(truth[:2], pred[:2]); total.add(truth[2], pred[2])
    one = evaluate.Agreement(6, 'cpu')
    one.add(truth, pred)
    a, b = total.result(), one.result()
    assert torch.equal(a['matrix'], b['matrix']) and torch.equal(a['boundary_counts'], b['boundary_counts']) and a['frames'] == b['frames'] == 3
    assert a['miou'] == b['miou'] and a['boundary'] == b['boundary'] and torch.equal(a['matrix'].view(-1), whole[:-1])


@pytest.mark.parametrize('name', NAMES)
def test_boundary_equals_four_shifted_copies(name):
    from pix2pix3d_amd import evaluate
    truth, pred, n = _maps()[name]
    for m in (truth, pred):
        got = evaluate.boundary(m)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), oracle_boundary(m.numpy()))
    if name == 'single label':
        assert bool((evaluate.boundary(truth) == 255).all())
    if name == 'checkerboard':
        assert torch.equal(evaluate.boundary(truth), truth)                              # no two neighbours are equal


def test_a_255_pixel_is_no_boundary_pixel_but_differs_from_its_neighbours():
    from pix2pix3d_amd import evaluate
    m = torch.full([5, 5], 3, dtype=torch.uint8)
    m[2, 2] = 255
    b = evaluate.boundary(m)
    want = torch.full([5, 5], 255, dtype=torch.uint8)
    want[1, 2] = want[3, 2] = want[2, 1] = want[2, 3] = 3
    assert torch.equal(b, want)


@pytest.mark.parametrize('name', NAMES)
def test_distance_histogram_and_boundary_counts_equal_brute_force(name):
    from pix2pix3d_amd import evaluate, regions
    truth, pred, n = _maps()[name]
    small_t, small_p = truth[:37, :53].contiguous(), pred[:37, :53].contiguous()           # brute force over EVERY boundary pixel: a corner of the blobs
    every = evaluate.CLASS_AGNOSTIC
    for sites, bins, (a, b) in ((every, 65, (small_t, small_p)), ((1,), 1, (truth, pred)), ((1, 4), 10, (truth, pred)), ((), 65, (truth, pred)),
                                (every, 4096, (small_t, small_p))):
        bt, bp = evaluate.boundary(a), evaluate.boundary(b)
        near = regions.nearest(bt, sites)
        assert np.array_equal(near.numpy(), brute_nearest(bt.numpy(), sites))
        hist = evaluate.distance_histogram(bp, sites, near, bins)
        assert hist.dtype == torch.int64 and np.array_equal(hist.numpy(), oracle_histogram(bp.numpy(), sites, near.numpy(), bins)), (sorted(sites)[:3], bins)
        assert int(hist.sum()) == int(np.isin(bp.numpy(), sorted(sites)).sum())
    counts = evaluate.boundary_counts(small_t, small_p)
    assert tuple(counts.shape) == (2, 67) and np.array_equal(counts.numpy(), oracle_boundary_counts(small_t.numpy(), small_p.numpy(), every, 65))
    per_class = evaluate.boundary_counts(truth, pred, n_labels=n, bins=20, per_class=True)
    assert tuple(per_class.shape) == (n, 2, 22)
    for c in range(n):
        assert np.array_equal(per_class[c].numpy(), oracle_boundary_counts(truth.numpy(), pred.numpy(), (c,), 20)), c


def test_an_empty_site_set_and_a_map_without_sites_land_in_the_last_slots():
    from pix2pix3d_amd import evaluate, regions
    truth, pred, _ = _maps()['blobs 6']
    bt, bp = evaluate.boundary(truth), evaluate.boundary(pred)
    assert int(evaluate.distance_histogram(bp, (), regions.nearest(bt, ()), 65).sum()) == 0       # nothing is in the empty set
    none = evaluate.distance_histogram(bp, evaluate.CLASS_AGNOSTIC, regions.nearest(bt, ()), 65)       # pixels in the set, no site anywhere
    assert int(none[-1]) == int((bp != 255).sum()) > 0 and int(none[:-1].sum()) == 0
    far = evaluate.distance_histogram(bp, evaluate.CLASS_AGNOSTIC, regions.nearest(bt, evaluate.CLASS_AGNOSTIC), 1)
    assert int(far[2]) == 0 and int(far[0]) + int(far[1]) == int((bp != 255).sum()) and int(far[1]) > 0
    out = torch.zeros(67, dtype=torch.int64)
    evaluate.distance_histogram(bp, evaluate.CLASS_AGNOSTIC, regions.nearest(bt, ()), 65, out=out)
    evaluate.distance_histogram(bp, evaluate.CLASS_AGNOSTIC, regions.nearest(bt, ()), 65, out=out)
    assert torch.equal(out, 2 * none)


# ---- 2. the metrics ------------------------------------------------------------------------------------------------------------------
def _close(a, b):
    return np.allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=1e-12, atol=0, equal_nan=True)       # two orders of fp64 division


@pytest.mark.parametrize('name', ['blobs 6', 'blobs 19', 'checkerboard', '1x300'])
def test_metrics_equal_the_textbook_formulas(name):
    from pix2pix3d_amd import evaluate
    truth, pred, n = _maps()[name]
    pred = torch.where(torch.from_numpy(np.random.RandomState(1).rand(*truth.shape) < 0.5), truth, pred)       # half right
    m = evaluate.metrics_from_confusion(evaluate.confusion(truth, pred, n))
    want = textbook_metrics(truth.numpy(), pred.numpy(), n)
    print(name, {k: m[k] for k in ('accuracy', 'miou', 'fw_iou')})
    for key in ('accuracy', 'iou', 'dice', 'miou', 'fw_iou'):
        assert _close(m[key], want[key]), key
    assert m['pixels'] == want['pixels'] == truth.numel() and m['left_out'] == 0 and type(m['accuracy']) is float and type(m['iou']) is list
    assert m['matrix'].dtype == torch.int64 and tuple(m['matrix'].shape) == (n, n) and int(m['matrix'].sum()) == m['pixels']
    hist = evaluate.boundary_counts(truth, pred)
    for tolerance in (0, 1, 2, 5):
        b = evaluate.metrics_from_boundary(hist, tolerance)
        assert _close([b['precision'], b['recall'], b['f_score']], textbook_f(hist.numpy(), tolerance)), tolerance
    rows = hist.numpy().astype(np.float64)
    d = np.sqrt(np.minimum(np.arange(67), 65).astype(np.float64))
    d[66] = math.sqrt(65)
    assert _close(evaluate.metrics_from_boundary(hist, 2)['chamfer'], ((rows[0] * d).sum() / rows[0].sum() + (rows[1] * d).sum() / rows[1].sum()) / 2)


def test_equal_maps_are_perfect():
    from pix2pix3d_amd import evaluate
    for name in ('blobs 6', 'blobs 19', 'checkerboard'):
        truth, _, n = _maps()[name]
        total = evaluate.Agreement(n, 'cpu')
        total.add(truth, truth.clone())
        r = total.result()
        assert r['accuracy'] == 1.0 and r['miou'] == 1.0 and r['fw_iou'] == 1.0 and r['boundary']['f_score'] == 1.0 and r['boundary']['chamfer'] == 0.0
        assert r['boundary']['precision'] == r['boundary']['recall'] == 1.0 and r['n_labels'] == n and all(v == 1.0 or math.isnan(v) for v in r['iou'])
    ink = (random_mask(1, 40, 40, 2, seed=3)[0] * 255).to(torch.uint8)
    m = evaluate.ink_agreement(ink, ink.clone())
    assert m['f_score'] == 1.0 and m['chamfer'] == 0.0 and m['ink_a'] == m['ink_b'] == int((ink == 255).sum())


def test_a_shift_by_three_pixels_is_outside_tolerance_two_and_inside_three():
    """Two labels on either side of a vertical edge, and the same map moved 3 pixels to the right.  The boundary of CLASS c is one pixel wide (the pixels of c
    beside the other label), so every truth boundary pixel is exactly 3 pixels from the pred boundary of its class: recall and precision 0 at tolerance 2,
    1 at tolerance 3.  The same holds for one-pixel ink lines.  The class-agnostic boundary is both sides of the edge, two pixels wide: its inner column is
    2 pixels from the other map's, its outer column 3 — half of it is within tolerance 2, by the same arithmetic."""
    from pix2pix3d_amd import evaluate
    truth = torch.zeros(32, 40, dtype=torch.uint8)
    truth[:, 17:] = 1
    pred = torch.zeros(32, 40, dtype=torch.uint8)
    pred[:, 20:] = 1
    per_class = evaluate.boundary_counts(truth, pred, n_labels=2, per_class=True)
    for m2, m3 in zip(evaluate.metrics_from_boundary(per_class, 2), evaluate.metrics_from_boundary(per_class, 3)):
        assert (m2['recall'], m2['precision'], m2['f_score']) == (0.0, 0.0, 0.0) and (m3['recall'], m3['precision'], m3['f_score']) == (1.0, 1.0, 1.0)
        assert m2['chamfer'] == 3.0 and m2['truth_pixels'] == m2['pred_pixels'] == 32
    ink_a, ink_b = torch.zeros(32, 40, dtype=torch.uint8), torch.zeros(32, 40, dtype=torch.uint8)
    ink_a[:, 17], ink_b[:, 20] = 255, 255
    assert evaluate.ink_agreement(ink_a, ink_b, tolerance=2)['recall'] == 0.0 and evaluate.ink_agreement(ink_a, ink_b, tolerance=3)['recall'] == 1.0
    assert evaluate.ink_agreement(ink_a, ink_b, tolerance=2)['ink_a'] == 32
    both = evaluate.boundary_counts(truth, pred)
    assert evaluate.metrics_from_boundary(both, 2)['recall'] == 0.5 and evaluate.metrics_from_boundary(both, 3)['recall'] == 1.0
    assert evaluate.metrics_from_boundary(both, 1)['recall'] == 0.0 and evaluate.metrics_from_boundary(both, 2)['chamfer'] == 2.5


def test_the_nan_conventions():
    from pix2pix3d_amd import evaluate
    truth, pred = torch.zeros(8, 8, dtype=torch.uint8), torch.zeros(8, 8, dtype=torch.uint8)
    pred[:, 4:] = 2
    m = evaluate.metrics_from_confusion(evaluate.confusion(truth, pred, 4))
    assert m['iou'][0] == 0.5 and m['iou'][2] == 0.0 and math.isnan(m['iou'][1]) and math.isnan(m['iou'][3]) and math.isnan(m['dice'][1])
    assert m['miou'] == 0.25 and m['fw_iou'] == 0.5 and m['accuracy'] == 0.5                  # classes 0 and 2 are present; only 0 in the truth
    empty = evaluate.metrics_from_confusion(torch.zeros(17, dtype=torch.int64))
    assert all(math.isnan(empty[k]) for k in ('accuracy', 'miou', 'fw_iou')) and empty['pixels'] == 0
    b = evaluate.metrics_from_boundary(evaluate.boundary_counts(truth, pred), 2)          # the truth has no boundary: recall NaN, precision 0, no exception
    assert math.isnan(b['recall']) and b['precision'] == 0.0 and math.isnan(b['f_score']) and math.isnan(b['chamfer']) and b['truth_pixels'] == 0
    z = evaluate.metrics_from_boundary(torch.zeros(2, 67, dtype=torch.int64), 2)
    assert math.isnan(z['precision']) and math.isnan(z['recall']) and math.isnan(z['f_score'])
    unused = evaluate.Agreement(6, 'cpu').result()
    assert math.isnan(unused['miou']) and math.isnan(unused['ink']['f_score']) and unused['frames'] == 0


def test_every_value_error():
    from pix2pix3d_amd import evaluate, regions
    t, p = torch.zeros(8, 9, dtype=torch.uint8), torch.zeros(8, 9, dtype=torch.uint8)
    near = regions.nearest(t, (0,))
    calls = [lambda: evaluate.confusion(t, p[:, :8], 4), lambda: evaluate.confusion(t, p[None], 4), lambda: evaluate.confusion(t, p, 0),
             lambda: evaluate.confusion(t, p, 33), lambda: evaluate.confusion(t.float(), p, 4), lambda: evaluate.confusion(t, p, 4, valid=p[:4]),
             lambda: evaluate.confusion(t, p, 4, out=torch.zeros(16, dtype=torch.int64)), lambda: evaluate.confusion(t, p, 4, out=torch.zeros(17)),
             lambda: evaluate.confusion(t.t(), p.t(), 4), lambda: evaluate.boundary(t.float()), lambda: evaluate.boundary(t[None]),
             lambda: evaluate.distance_histogram(t, (0,), near, 0), lambda: evaluate.distance_histogram(t, (0,), near, 4097),
             lambda: evaluate.distance_histogram(t, (256,), near, 8), lambda: evaluate.distance_histogram(t, (0,), near.long(), 8),
             lambda: evaluate.distance_histogram(t, (0,), near[:4], 8), lambda: evaluate.distance_histogram(t, (0,), near, 8, out=torch.zeros(9, dtype=torch.int64)),
             lambda: evaluate.boundary_counts(t, p[:4]), lambda: evaluate.boundary_counts(t, p, per_class=True), lambda: evaluate.boundary_counts(t, p, bins=0),
             lambda: evaluate.metrics_from_boundary(torch.zeros(2, 67, dtype=torch.int64), 9), lambda: evaluate.metrics_from_boundary(torch.zeros(2, 67, dtype=torch.int64), -1),
             lambda: evaluate.metrics_from_boundary(torch.zeros(3, 67, dtype=torch.int64), 2), lambda: evaluate.metrics_from_confusion(torch.zeros(16, dtype=torch.int64)),
             lambda: evaluate.ink_counts(t, p[:4]), lambda: evaluate.ink_counts(t, p, threshold=0), lambda: evaluate.ink_counts(t, p, threshold=256),
             lambda: evaluate.Agreement(0, 'cpu'), lambda: evaluate.Agreement(6, 'cpu', bins=5000)]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    assert evaluate.metrics_from_boundary(torch.zeros(2, 67, dtype=torch.int64), 8)['pred_pixels'] == 0          # 8^2 = 64 < 65 is the largest tolerance


# ---- 3. the binding ------------------------------------------------------------------------------------------------------------------
def test_the_headers_nine_names_are_in_order_and_its_constants_are_pinned():
    from pix2pix3d_amd import evaluate, regions
    names = list(regions.HEADER.functions)
    assert names == ['p3d_label_components', 'p3d_label_nearest', 'p3d_label_warp', 'p3d_label_confusion', 'p3d_label_boundary', 'p3d_label_distance_histogram',
                     'p3d_view_splat', 'p3d_view_resolve', 'p3d_view_difference_histogram']
    assert regions.HEADER.constants == {'P3D_LABEL_MAX_LINEAR_LOG2': 22, 'P3D_LABEL_MAX_TRANSLATION_LOG2': 40, 'P3D_LABEL_MAX_LABELS': 32, 'P3D_LABEL_MAX_BINS': 4096, 'P3D_LABEL_MAX_FRAMES': 65536, 'P3D_VIEW_MAX_RADIUS': 2,
                                     'P3D_VIEW_MAX_CHANNELS': 4, 'P3D_VIEW_GUARD': 4, 'P3D_VIEW_MAX_TOLERANCE': (1 << 31) - 1, 'P3D_VIEW_EMPTY': (1 << 63) - 1, 'P3D_VIEW_HOLE': 0,
                                     'P3D_VIEW_CONSISTENT': 1, 'P3D_VIEW_BEHIND': 2, 'P3D_VIEW_IN_FRONT': 3, 'P3D_VIEW_NO_TARGET': 4}
    assert not regions.HEADER.structs
    assert (evaluate.MAX_LABELS, evaluate.MAX_BINS, evaluate.MAX_FRAMES) == (32, 4096, 65536)
    assert len(regions.HEADER.functions['p3d_label_confusion'][1]) == 15 and len(regions.HEADER.functions['p3d_label_distance_histogram'][1]) == 9
    L = regions.regions_lib()
    assert all(getattr(L, n) is not None for n in names)


def test_argument_errors_of_the_new_entry_points_come_back_as_codes_without_a_gpu():
    """The checks run before any device call: the library is needed, a GPU is not."""
    from pix2pix3d_amd import _lib, regions
    L, E = regions.regions_lib(), _lib.P3D_ERR_ARGUMENT
    n0 = regions.launch_count()
    buf = (ctypes.c_uint8 * 8192)()
    p = ctypes.addressof(buf)
    p += -p % 8
    words = (ctypes.c_uint32 * 8)()

    def err(code, text):
        assert code == E == -2 and text in L.p3d_last_error(), (code, L.p3d_last_error())
    conf = lambda t=p, tr=8, tf=64, q=p + 1024, qr=8, qf=64, v=None, vr=0, vf=0, n=2, h=8, w=8, c=4, out=p + 4096: \
        L.p3d_label_confusion(t, tr, tf, q, qr, qf, v, vr, vf, n, h, w, c, out, None)
    err(conf(t=None), b'non-null')
    err(conf(q=None), b'non-null')
    err(conf(out=None), b'non-null')
    err(conf(c=0), b'n_labels')
    err(conf(c=33), b'n_labels')
    err(conf(n=-1), b'frames')
    err(conf(n=65537), b'frames')
    err(conf(h=0), b'a side')
    err(conf(w=4097), b'a side')
    err(conf(tr=7), b'row pitch')
    err(conf(v=p + 2048, vr=7, vf=64), b'row pitch')
    err(conf(qf=63), b'frame pitch')
    err(conf(v=p + 2048, vr=8, vf=8), b'frame pitch')
    err(conf(out=p + 4097), b'aligned')
    assert conf(n=0) == 0 and conf(n=0, t=None, q=None, out=None) == 0                         # no frames: a success that launches nothing
    err(L.p3d_label_boundary(None, 8, p + 1024, 8, 8, 8, None), b'non-null')
    err(L.p3d_label_boundary(p, 8, None, 8, 8, 8, None), b'non-null')
    err(L.p3d_label_boundary(p, 8, p + 1024, 8, 0, 8, None), b'a side')
    err(L.p3d_label_boundary(p, 7, p + 1024, 8, 8, 8, None), b'row pitch')
    err(L.p3d_label_boundary(p, 8, p + 1024, 7, 8, 8, None), b'row pitch')
    err(L.p3d_label_boundary(p, 8, p, 8, 8, 8, None), b'out of place')
    err(L.p3d_label_boundary(p, 8, p + 63, 8, 8, 8, None), b'overlap')
    err(L.p3d_label_boundary(p + 63, 8, p, 8, 8, 8, None), b'overlap')
    hist = lambda f=p, fp=8, s=words, near=p + 1024, bins=65, out=p + 4096, h=8, w=8: L.p3d_label_distance_histogram(f, fp, s, near, bins, out, h, w, None)
    err(hist(f=None), b'non-null')
    err(hist(s=None), b'non-null')
    err(hist(near=None), b'non-null')
    err(hist(out=None), b'non-null')
    err(hist(h=4097), b'a side')
    err(hist(fp=7), b'row pitch')
    err(hist(bins=0), b'bins')
    err(hist(bins=4097), b'bins')
    err(hist(near=p + 1025), b'aligned')
    err(hist(out=p + 4100), b'aligned')
    assert regions.launch_count() == n0
