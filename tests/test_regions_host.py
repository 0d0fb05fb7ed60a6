"""pix2pix3d_amd.regions without a GPU: the torch formulations (the definition of every result byte) against first principles — scipy's labelling, a brute-force
nearest site, scipy's distance transform and dilation, slice copies and rot90 —, a session with a mixed log on a small CPU generator, and the binding of
libp3d_regions.so.  Every comparison is integer equality."""
import ctypes
import pathlib
import re

import numpy as np
import pytest
import torch

from model_cases import build_generator
from edit_cases import oracle_paint, random_mask, demo_pose
from regions_cases import spiral, checkerboard, scipy_components, brute_nearest, disc

ROOT = pathlib.Path(__file__).resolve().parent.parent


# ---- 1. components ----------------------------------------------------------------------------------------------------------------
def _component_masks():
    return {'blobs 37x41': random_mask(1, 37, 41, 6, seed=1)[0], 'blobs 64x64': random_mask(1, 64, 64, 19, seed=2)[0], 'checkerboard': checkerboard(12, 15),
            'spiral 33': spiral(33), '1x1': torch.full([1, 1], 7, dtype=torch.uint8), '1x50': random_mask(1, 1, 50, 3, seed=3)[0],
            '50x1': random_mask(1, 50, 1, 3, seed=4)[0]}


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('name', sorted(_component_masks()))
def test_components_equal_scipy_label_per_label(name, connectivity):
    from pix2pix3d_amd import regions
    mask = _component_masks()[name]
    ids = regions.components(mask, connectivity)
    want = scipy_components(mask.numpy(), connectivity)
    assert ids.dtype == torch.int32 and ids.is_contiguous() and tuple(ids.shape) == tuple(mask.shape)
    bad = int((ids.numpy() != want).sum())
    print(name, connectivity, 'components', len(np.unique(want)), 'differing ids', bad)
    assert bad == 0
    flat = ids.numpy().ravel()
    assert (flat[flat] == flat).all() and (flat <= np.arange(flat.size)).all()          # every id is a pixel of its own part, the smallest one


def test_the_two_neighbourhoods_differ_on_a_checkerboard_and_agree_on_the_spiral():
    from pix2pix3d_amd import regions
    board = checkerboard(12, 15)
    four, eight = regions.components(board, 4), regions.components(board, 8)
    assert len(four.unique()) == 12 * 15 and len(eight.unique()) == 2
    chain = spiral(33)
    assert len(regions.components(chain, 4).unique()) == 2 and torch.equal(regions.components(chain, 4), regions.components(chain, 8))
    with pytest.raises(ValueError):
        regions.components(board, 6)
    with pytest.raises(ValueError):
        regions.components(board.float(), 4)


# ---- 2. nearest ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', [0, 1, 3, -1])
@pytest.mark.parametrize('size', [(1, 1), (23, 31), (5, 29), (30, 5), (31, 31)])
def test_nearest_equals_brute_force_under_the_d2_index_rule(size, radius):
    from pix2pix3d_amd import regions
    h, w = size
    mask = random_mask(1, h, w, 6, seed=h * w)[0]
    mask[h // 2, w // 3] = 9                                                    # a lone site besides the blobs
    for sites in ({2, 9}, {9}, set(), set(range(256))):
        got = regions.nearest(mask, sites, radius)
        want = brute_nearest(mask.numpy(), sites, radius)
        assert got.dtype == torch.int32 and got.is_contiguous() and np.array_equal(got.numpy(), want), (size, radius, sorted(sites)[:3])
    assert (regions.nearest(mask, set(), radius) == -1).all()
    assert torch.equal(regions.nearest(mask, set(range(256)), radius), torch.arange(h * w, dtype=torch.int32).view(h, w))


def test_nearest_distances_equal_the_euclidean_distance_transform():
    from scipy import ndimage
    from pix2pix3d_amd import regions
    mask = random_mask(1, 64, 64, 6, seed=9)[0]
    near = regions.nearest(mask, {1, 4}).long()
    ys, xs = torch.arange(64)[:, None], torch.arange(64)[None, :]
    d2 = (near // 64 - ys) ** 2 + (near % 64 - xs) ** 2
    edt = ndimage.distance_transform_edt(~np.isin(mask.numpy(), [1, 4]))
    assert np.array_equal(d2.numpy(), np.rint(edt ** 2).astype(np.int64))
    assert bool(np.isin(mask.view(-1)[near.view(-1)].numpy(), [1, 4]).all())


def test_a_tie_goes_to_the_smaller_index():
    from pix2pix3d_amd import regions
    mask = torch.zeros(9, 9, dtype=torch.uint8)
    mask[4, 1] = mask[4, 7] = mask[1, 4] = 5                                    # (4, 4) is 3 pixels from all three
    near = regions.nearest(mask, {5})
    assert int(near[4, 4]) == 1 * 9 + 4 and int(near[5, 4]) == 4 * 9 + 1         # row 5: the upper site is farther, left and right tie: the left one
    assert int(near[4, 1]) == 4 * 9 + 1
    with pytest.raises(ValueError):
        regions.nearest(mask, {256})


# ---- 3. grow / shrink / remove ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [1, 4, 9])
def test_grow_is_binary_dilation_by_the_disc(r):
    from scipy import ndimage
    from pix2pix3d_amd import regions
    mask = random_mask(1, 48, 61, 6, seed=30 + r)[0]
    out = regions.grow(mask, 2, r)
    grown = ndimage.binary_dilation(mask.numpy() == 2, structure=disc(r))
    assert np.array_equal(out.numpy() == 2, grown) and np.array_equal(out.numpy()[~grown], mask.numpy()[~grown])
    only = regions.grow(mask, 2, r, over={0, 1})
    allowed = np.isin(mask.numpy(), [0, 1])
    assert np.array_equal(only.numpy(), np.where(grown & allowed, 2, mask.numpy()))
    assert bool((only[~torch.from_numpy(allowed)] == mask[~torch.from_numpy(allowed)]).all())          # protected labels stay
    assert torch.equal(regions.grow(mask, 77, r), mask)                          # a label that does not occur


def test_shrink_grow_and_remove_create_no_label():
    from pix2pix3d_amd import regions
    mask = random_mask(1, 48, 61, 6, seed=40)[0]
    present = set(mask.unique().tolist())
    eroded = regions.shrink(mask, 3, 3)
    assert set(eroded.unique().tolist()) <= present and int((eroded == 3).sum()) < int((mask == 3).sum())
    assert bool((eroded[mask != 3] == mask[mask != 3]).all())
    again = regions.grow(eroded, 3, 3)
    assert set(again.unique().tolist()) <= present
    gone = regions.remove(mask, 3)
    assert int((gone == 3).sum()) == 0 and set(gone.unique().tolist()) == present - {3} and bool((gone[mask != 3] == mask[mask != 3]).all())
    alone = torch.full([7, 9], 3, dtype=torch.uint8)
    assert torch.equal(regions.remove(alone, 3), alone)                          # the only label stays
    assert torch.equal(regions.remove(mask, 77), mask)


def test_select_flood_fill_and_bbox():
    from pix2pix3d_amd import regions
    mask = torch.zeros(20, 30, dtype=torch.uint8)
    mask[3:9, 4:11] = 2
    mask[12:15, 20:29] = 2
    region = regions.select(mask, 5, 4)
    assert region.dtype == torch.bool and torch.equal(region, (mask == 2) & (torch.arange(20)[:, None] < 10))
    assert regions.bbox(region) == (4, 3, 10, 8) and regions.bbox(mask == 9) is None
    filled = regions.flood_fill(mask, 25, 13, 7)
    assert int((filled == 7).sum()) == 27 and torch.equal(filled[:10], mask[:10])
    with pytest.raises(ValueError):
        regions.select(mask, 30, 0)


# ---- 4. affine_coef and warp ------------------------------------------------------------------------------------------------------
def test_identity_translation_and_rotation():
    from pix2pix3d_amd import regions
    mask = random_mask(1, 41, 41, 6, seed=50)[0]
    region = mask == 2
    under = torch.full_like(mask, 9)
    assert regions.affine_coef([[1, 0, 0], [0, 1, 0]]) == (65536, 0, 0, 0, 65536, 0)
    same = regions.warp(mask, region, under, regions.affine_coef(np.eye(2, 3)))
    assert torch.equal(same, torch.where(region, mask, under))
    coef = regions.affine_coef([[1, 0, 5], [0, 1, -3]])
    assert coef == (65536, 0, -5 * 65536, 0, 65536, 3 * 65536)
    moved = regions.warp(mask, region, under, coef)
    want = under.clone()
    want[:38, 5:] = torch.where(region[3:, :36], mask[3:, :36], under[:38, 5:])   # a slice copy
    assert torch.equal(moved, want)
    c = 20                                                                      # 90 degrees about the pixel centre (20, 20): (x, y) -> (c - (y - c), c + (x - c))
    turned = regions.warp(mask, region, under, regions.affine_coef([[0, -1, 2 * c], [1, 0, 0]]))
    assert torch.equal(turned, torch.where(torch.rot90(region, -1, [0, 1]), torch.rot90(mask, -1, [0, 1]), under))
    by_angle = regions.affine_coef([[np.cos(np.pi / 2), -np.sin(np.pi / 2), 2 * c], [np.sin(np.pi / 2), np.cos(np.pi / 2), 0]])
    assert by_angle == regions.affine_coef([[0, -1, 2 * c], [1, 0, 0]])
    assert all(isinstance(v, int) for v in coef)


def test_singular_and_oversized_matrices_are_value_errors():
    from pix2pix3d_amd import regions
    for bad in ([[1, 2, 0], [2, 4, 0]], [[0, 0, 0], [0, 0, 0]], [[1e-3, 0, 0], [0, 1, 0]], [[1, 0, 1e8], [0, 1, 0]], [[1, 0, float('nan')], [0, 1, 0]],
                [[1, 0], [0, 1]]):
        with pytest.raises(ValueError):
            regions.affine_coef(bad)
    assert regions.affine_coef([[1 / 64, 0, 0], [0, 1, 0]])[0] == 1 << 22          # the largest linear integer
    m = torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError):
        regions.warp(m, m == 0, m.clone(), (1 << 23, 0, 0, 0, 65536, 0))
    with pytest.raises(ValueError):
        regions.warp(m, m == 0, m.clone(), (65536, 0, 0, 0, 65536, 0), out=m)


def test_transform_vacates_fills_and_pastes():
    from pix2pix3d_amd import regions
    mask = torch.zeros(24, 24, dtype=torch.uint8)
    mask[:, 12:] = 1
    mask[8:12, 8:16] = 5                                                        # a block across the border of the two halves
    region = mask == 5
    up = regions.transform(mask, region, [[1, 0, 0], [0, 1, -6]])
    want = torch.zeros(24, 24, dtype=torch.uint8)
    want[:, 12:] = 1
    want[2:6, 8:16] = 5                                                         # vacated pixels took the nearest surroundings: the two halves again
    assert torch.equal(up, want)
    flat = regions.transform(mask, region, [[1, 0, 0], [0, 1, -6]], fill=3)
    want[8:12, 8:16] = 3
    assert torch.equal(flat, want)
    assert torch.equal(regions.transform(mask, mask == 9, [[2, 0, 0], [0, 2, 0]]), mask)      # an empty region
    with pytest.raises(ValueError):
        regions.transform(mask, region, np.eye(2, 3), fill='mean')


# ---- 5. a session with a mixed log ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def loaded():
    """(G, res, base mask, pose): shared, never modified — the small generator of tests/test_edit_host.py."""
    G = build_generator('seg2cat', 'cpu', cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0)
    res = G.backbone.mapping.in_resolution
    return G, res, random_mask(1, res, res, 6, seed=4)[0], torch.from_numpy(demo_pose(G))


def test_a_mixed_log_equals_the_functions_by_hand_and_undo_walks_it_back(loaded):
    from pix2pix3d_amd import edit, regions
    G, res, base, pose = loaded
    s = edit.EditSession(G, neural_rendering_resolution=16)
    s.load(base, pose)
    a, b = [(5, 5, res - 6, res // 2, 7, 1)], [(res // 2, 3, res // 2, res - 4, 5, 2), (3, res - 8, res - 3, res - 8, 3, 4)]
    label = int(base[res // 2, res // 4])
    states = [base]
    s.paint(a); states.append(torch.from_numpy(oracle_paint(states[-1].numpy(), a)))
    s.fill(3, res - 3, 5, connectivity=8); states.append(regions.flood_fill(states[-1], 3, res - 3, 5, 8))
    assert torch.equal(s.mask, states[-1])
    s.paint(b); states.append(torch.from_numpy(oracle_paint(states[-1].numpy(), b)))
    box = regions.bbox(states[-1] == 1)
    cx, cy = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2
    s.scale(1, 1.5)
    states.append(regions.transform(states[-1], states[-1] == 1, [[1.5, 0, cx - 1.5 * cx], [0, 1.5, cy - 1.5 * cy]]))
    s.remove(label); states.append(regions.remove(states[-1], label))
    assert torch.equal(s.mask, states[-1]) and len(s.log) == 5 and [e[0] for e in s.log] == ['paint', 'fill', 'paint', 'warp', 'shrink']
    kind, spec, coef, fill = s.log[3]
    assert spec == 1 and fill == 'nearest' and len(coef) == 6 and all(type(v) is int for v in coef)          # integers, no float and no centre
    assert coef == regions.affine_coef([[1.5, 0, cx - 1.5 * cx], [0, 1.5, cy - 1.5 * cy]])
    assert len(s.strokes) == 3 and torch.equal(s.strokes, edit.stroke_table(a + b))
    assert len({int(v) for st in states for v in st.unique()} - set(range(6))) == 0
    for want in reversed(states[:-1]):                                         # undo pops one entry of any kind
        s.undo()
        assert torch.equal(s.mask, want)
    assert len(s.log) == 0 and s.mask is s._base
    s.undo()
    assert torch.equal(s.mask, base)
    replayed = edit.EditSession(G, neural_rendering_resolution=16)              # the same log, never looked at in between: one pass from the base
    replayed.load(base, pose)
    replayed.paint(a); replayed.fill(3, res - 3, 5, connectivity=8); replayed.paint(b); replayed.scale(1, 1.5, centre=(cx, cy)); replayed.remove(label)
    assert torch.equal(replayed.mask, states[-1])
    replayed.clear()
    assert torch.equal(replayed.mask, base) and len(replayed.log) == 0


def test_region_methods_validate_on_the_host_and_resolve_components_when_applied(loaded):
    from pix2pix3d_amd import edit, regions
    G, res, base, pose = loaded
    s = edit.EditSession(G, neural_rendering_resolution=16)
    with pytest.raises(RuntimeError):
        s.fill(0, 0, 1)
    s.load(base, pose)
    for call in (lambda: s.fill(res, 0, 1), lambda: s.fill(0, 0, 6), lambda: s.fill(0, 0, 1, connectivity=5), lambda: s.grow(6, 2), lambda: s.grow(1, -1),
                 lambda: s.grow(1, 2, over={7}), lambda: s.shrink(1, 1.5), lambda: s.remove(-1), lambda: s.move(9, 1, 1), lambda: s.move(('blob', 1, 1), 1, 1),
                 lambda: s.scale(1, 0.0), lambda: s.transform(1, [[1, 0, 0], [0, 1, 0]], fill=6), lambda: s.transform(1, np.eye(2, 3), fill='mean')):
        with pytest.raises(ValueError):
            call()
    assert len(s.log) == 0 and s.mask is s._base
    x, y = res // 2, res // 2
    s.move(('component', x, y), 3, -2)
    region = regions.select(base, x, y)
    assert s.log[0][1] == ('component', x, y, 4) and torch.equal(s.mask, regions.transform(base, region, [[1, 0, 3], [0, 1, -2]]))
    s.rotate(int(base[y, x]), 90, centre=(x, y))
    turned = regions.transform(s._mask_after(1), s._mask_after(1) == int(base[y, x]), [[0, -1, x + y], [1, 0, y - x]])
    assert torch.equal(s.mask, turned)
    s.grow(2, 2, over=[0, 1]); s.shrink(3, 1)
    assert torch.equal(s.mask, regions.shrink(regions.grow(turned, 2, 2, over={0, 1}), 3, 1))


def test_a_stroke_only_session_paints_once_per_change_and_equals_the_oracle(loaded, monkeypatch):
    from pix2pix3d_amd import edit
    G, res, base, pose = loaded
    calls = []
    real = edit.paint_strokes
    monkeypatch.setattr(edit, 'paint_strokes', lambda *a, **k: calls.append(len(a[1])) or real(*a, **k))
    a, b = [(10, 10, res - 10, res - 10, 11, 4)], [(res - 10, 10, 10, res - 10, 11, 1), (res // 2, 0, res // 2, res, 3, 0)]
    for replay, order in (('time', a + b), ('label', [b[1], b[0], a[0]])):
        s = edit.EditSession(G, neural_rendering_resolution=16, replay=replay)
        s.load(base, pose)
        del calls[:]
        assert s.mask is s._base and calls == []
        s.paint(a)
        assert torch.equal(s.mask, torch.from_numpy(oracle_paint(base.numpy(), a))) and s.mask is s.mask and calls == [1]
        s.paint(b)
        assert torch.equal(s.mask, torch.from_numpy(oracle_paint(base.numpy(), order))) and calls == [1, 3]      # the whole run, one launch
        assert torch.equal(s.strokes, edit.stroke_table(order))
        s.undo()
        assert torch.equal(s.mask, torch.from_numpy(oracle_paint(base.numpy(), a))) and calls == [1, 3]          # the kept mask: nothing runs
        s.paint(b); s.grow(4, 1)
        s.mask
        assert calls == [1, 3, 3]
        s.undo()
        assert torch.equal(s.mask, torch.from_numpy(oracle_paint(base.numpy(), order))) and calls == [1, 3, 3]


def test_kept_masks_are_bounded_and_older_entries_replay(loaded):
    from pix2pix3d_amd import edit, regions
    G, res, base, pose = loaded
    s = edit.EditSession(G, neural_rendering_resolution=16)
    s.load(base, pose)
    want = [base]
    for k in range(40):
        s.grow(k % 6, 1) if k % 2 else s.paint([(k, k, k + 9, k + 2, 3, k % 6)])
        want.append(regions.grow(want[-1], k % 6, 1) if k % 2 else torch.from_numpy(oracle_paint(want[-1].numpy(), [(k, k, k + 9, k + 2, 3, k % 6)])))
        assert torch.equal(s.mask, want[-1])
    assert len(s._kept) == s.KEPT_MASKS == 32
    for k in range(39, 2, -1):
        s.undo()
    assert torch.equal(s.mask, want[3])                                         # older than every kept mask: replayed from the base


# ---- 6. the binding -------------------------------------------------------------------------------------------------------------
def test_regions_calls_its_three_entry_points_and_its_header_pins_names_and_constants():
    """Declared, exported by its own library alone, bound: the regions row of tests/test_side_libraries.py.  The header is the library's whole ABI: the
    region tools, the agreement metrics and the cross-view functions, with every bound and code they share with Python."""
    from pix2pix3d_amd import regions
    called = set(re.findall(r'\bregions_lib\(\)\.(p3d_\w+)', (ROOT / 'pix2pix3d_amd' / 'regions.py').read_text()))
    assert {'p3d_label_components', 'p3d_label_nearest', 'p3d_label_warp'} <= called
    assert list(regions.HEADER.functions) == ['p3d_label_components', 'p3d_label_nearest', 'p3d_label_warp', 'p3d_label_confusion', 'p3d_label_boundary', 'p3d_label_distance_histogram',
                                             'p3d_view_splat', 'p3d_view_resolve', 'p3d_view_difference_histogram']
    assert regions.HEADER.constants == {'P3D_LABEL_MAX_LINEAR_LOG2': 22, 'P3D_LABEL_MAX_TRANSLATION_LOG2': 40, 'P3D_LABEL_MAX_LABELS': 32, 'P3D_LABEL_MAX_BINS': 4096, 'P3D_LABEL_MAX_FRAMES': 65536, 'P3D_VIEW_MAX_RADIUS': 2,
                                     'P3D_VIEW_MAX_CHANNELS': 4, 'P3D_VIEW_GUARD': 4, 'P3D_VIEW_MAX_TOLERANCE': (1 << 31) - 1, 'P3D_VIEW_EMPTY': (1 << 63) - 1, 'P3D_VIEW_HOLE': 0,
                                     'P3D_VIEW_CONSISTENT': 1, 'P3D_VIEW_BEHIND': 2, 'P3D_VIEW_IN_FRONT': 3, 'P3D_VIEW_NO_TARGET': 4}
    assert not regions.HEADER.structs
    assert (regions.MAX_LINEAR, regions.MAX_TRANSLATION) == (1 << 22, 1 << 40)


def test_argument_errors_come_back_as_codes_without_a_gpu():
    """The checks run before any device call: the library is needed, a GPU is not."""
    from pix2pix3d_amd import _lib, regions
    L, E = regions.regions_lib(), _lib.P3D_ERR_ARGUMENT
    n0 = regions.launch_count()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    words, coef = (ctypes.c_uint32 * 8)(), (ctypes.c_int64 * 6)(65536, 0, 0, 0, 65536, 0)

    def err(code, text):
        assert code == E == -2 and text in L.p3d_last_error(), (code, L.p3d_last_error())
    err(L.p3d_label_components(None, 8, p, 8, 8, 4, None), b'non-null')
    err(L.p3d_label_components(p, 8, None, 8, 8, 4, None), b'non-null')
    err(L.p3d_label_components(p, 8, p + 1024, 8, 8, 6, None), b'connectivity')
    err(L.p3d_label_components(p, 8, p + 1024, 0, 8, 4, None), b'a side')
    err(L.p3d_label_components(p, 8, p + 1024, 8, 4097, 4, None), b'a side')
    err(L.p3d_label_components(p, 7, p + 1024, 8, 8, 4, None), b'row pitch')
    err(L.p3d_label_nearest(None, 8, words, -1, p + 1024, p + 2048, 8, 8, None), b'non-null')
    err(L.p3d_label_nearest(p, 8, None, -1, p + 1024, p + 2048, 8, 8, None), b'non-null')
    err(L.p3d_label_nearest(p, 8, words, -1, None, p + 2048, 8, 8, None), b'non-null')
    err(L.p3d_label_nearest(p, 8, words, -1, p + 1024, p + 2048, 8, 0, None), b'a side')
    err(L.p3d_label_nearest(p, 8, words, -1, p + 1024, p + 1024, 8, 8, None), b'workspace')
    err(L.p3d_label_warp(p, 8, p, 8, p, 8, None, 8, coef, 8, 8, None), b'non-null')
    err(L.p3d_label_warp(p, 8, p, 8, p, 8, p + 1024, 8, None, 8, 8, None), b'non-null')
    err(L.p3d_label_warp(p, 8, p, 8, p, 8, p + 1024, 8, coef, 0, 8, None), b'a side')
    err(L.p3d_label_warp(p, 8, p, 8, p, 8, p, 8, coef, 8, 8, None), b'out of place')
    coef[0] = (1 << 22) + 1
    err(L.p3d_label_warp(p, 8, p, 8, p, 8, p + 1024, 8, coef, 8, 8, None), b'coef[0]')
    assert regions.launch_count() == n0
