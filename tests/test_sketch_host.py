"""pix2pix3d_amd.sketch on the host: the torch formulations (the definitions) against independent numpy statements of the rules, the thinning table against
the Zhang-Suen conditions, and a CPU session on a small edge2car generator.  Every comparison is integer equality or equality of float bits."""
import os

import numpy as np
import pytest
import torch

from model_cases import build_generator
from edit_cases import demo_pose
from sketch_cases import (scene, random_grey, drawing, numpy_blur3, numpy_resize_nearest, script_condition, label_components, flood_components, numpy_link,
                          zhang_suen_deletable)


# ---- 1. blur3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(1, 1), (1, 7), (7, 1), (2, 2), (37, 53)])
def test_blur3_equals_reflect_padding_and_nine_slices(size):
    from pix2pix3d_amd import sketch
    ink = random_grey(size[0], size[1], seed=size[0] + size[1])
    got = sketch.blur3(ink)
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), numpy_blur3(ink.numpy()))


def test_a_blurred_one_pixel_line_takes_six_values():
    """k of the nine taps on the line: (255 k + 4) // 9 for k = 0 .. 5 (a line's end 1 and 2, its run 3, beside a crossing 4, the crossing 5)."""
    from pix2pix3d_amd import sketch
    ink, _ = drawing()
    assert set(ink.unique().tolist()) == {0, 255}
    assert set(sketch.blur3(ink).unique().tolist()) == {0, 28, 57, 85, 113, 142}


# ---- 2. condition --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('convention', ['dataset', 'input'])
@pytest.mark.parametrize('size, resolution', [((512, 512), 128), ((37, 53), 16), ((5, 3), 16)])
def test_condition_equals_the_scripts_expressions_on_the_prepared_mask(size, resolution, convention):
    """Integral (512 -> 128), non-integral (37 x 53 -> 16) and enlarging resizes; blur on and off; float BITS."""
    from pix2pix3d_amd import sketch
    ink = random_grey(size[0], size[1], seed=resolution)
    for blur in (True, False):
        prepared = numpy_resize_nearest(numpy_blur3(ink.numpy()) if blur else ink.numpy(), resolution)
        want = script_condition(prepared, convention)
        got = sketch.condition(ink, resolution, blur=blur, table=convention)
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, 1, resolution, resolution)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (size, resolution, convention, blur)
    assert torch.equal(sketch.condition(ink, resolution, table=sketch.condition_table(convention)), sketch.condition(ink, resolution, table=convention))


def test_tables_and_from_drawing():
    from pix2pix3d_amd import sketch
    v = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(sketch.condition_table('dataset'), -(v.float() / 127.5 - 1)) and float(sketch.condition_table('dataset')[255]) == -1.0
    assert torch.equal(sketch.condition_table('input'), (255 - v).float() / 127.5 - 1)
    assert torch.equal(sketch.from_drawing(v[None]), (255 - v)[None])
    with pytest.raises(ValueError):
        sketch.condition_table('files')


# ---- 3. edges ------------------------------------------------------------------------------------------------------------------------------
def _numpy_edge_classes(image, low, high, smooth):
    """The five steps of p3d_sketch.h in numpy loops over taps, int64; np.pad(mode='reflect') per step (sizes >= 3 only: pad 2 of an axis)."""
    g = np.asarray(image, np.int64)
    if g.ndim == 3:
        g = (77 * g[..., 0] + 150 * g[..., 1] + 29 * g[..., 2] + 128) >> 8
    h, w = g.shape
    if smooth:
        p = np.pad(g, 2, mode='reflect')
        k = np.array([1, 4, 6, 4, 1])
        v = sum(k[i] * k[j] * p[i:i + h, j:j + w] for i in range(5) for j in range(5))
        g = (v + 128) >> 8
    p = np.pad(g, 1, mode='reflect')
    t = lambda dy, dx: p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    gx = (t(-1, 1) + 2 * t(0, 1) + t(1, 1)) - (t(-1, -1) + 2 * t(0, -1) + t(1, -1))
    gy = (t(1, -1) + 2 * t(1, 0) + t(1, 1)) - (t(-1, -1) + 2 * t(-1, 0) + t(-1, 1))
    mag = np.abs(gx) + np.abs(gy)
    m = np.pad(mag, 1)
    out = np.zeros([h, w], np.uint8)
    for y in range(h):
        for x in range(w):
            ax, ay = abs(int(gx[y, x])), abs(int(gy[y, x])) << 15
            t22 = ax * 13573
            t67 = t22 + (ax << 16)
            c = int(mag[y, x])
            if ay < t22:
                kept = c > m[y + 1, x] and c >= m[y + 1, x + 2]
            elif ay > t67:
                kept = c > m[y, x + 1] and c >= m[y + 2, x + 1]
            else:
                s = -1 if (int(gx[y, x]) ^ int(gy[y, x])) < 0 else 1
                kept = c > m[y, x + 1 - s] and c > m[y + 2, x + 1 + s]
            out[y, x] = 2 if kept and c > high else (1 if kept and c > low else 0)
    return out


@pytest.fixture(scope='module')
def scene_classes():
    from pix2pix3d_amd import sketch
    rgb = scene()
    return rgb, sketch.edge_classes(rgb, 40, 120, smooth=True)


@pytest.mark.parametrize('smooth', [True, False])
def test_edge_classes_equal_a_numpy_statement_of_the_five_steps(smooth):
    from pix2pix3d_amd import sketch
    rgb = scene()
    grey = random_grey(23, 31, seed=9)
    for image, low, high in ((rgb, 40, 120), (grey, 100, 400), (grey, 0, 0), (grey, 2040, 2040)):
        got = sketch.edge_classes(image, low, high, smooth=smooth)
        assert np.array_equal(got.numpy(), _numpy_edge_classes(image.numpy(), low, high, smooth)), (tuple(image.shape), low, high)
    assert int(sketch.edge_classes(grey, 2040, 2040, smooth=smooth).max()) == 0


def test_hysteresis_on_the_scene_keeps_weak_edges_only_beside_strong_ones(scene_classes):
    from pix2pix3d_amd import sketch
    rgb, classes = scene_classes
    ink = sketch.link(classes)
    c = classes.numpy()
    ids, count = label_components(c != 0)
    with_strong = set(ids[c == 2].tolist())
    kept, dropped = int(((c == 1) & (ink.numpy() == 255)).sum()), int(((c == 1) & (ink.numpy() == 0)).sum())
    print('strong', int((c == 2).sum()), 'weak', int((c == 1).sum()), 'components', count, 'with a strong pixel', len(with_strong), 'weak kept', kept, 'dropped', dropped)
    assert set(ink.unique().tolist()) == {0, 255} and kept >= 1 and dropped >= 1
    assert set(ids[ink.numpy() == 255].tolist()) <= with_strong                # no kept pixel outside a component with a strong pixel
    assert np.array_equal(ink.numpy(), numpy_link(c))
    flood, n_flood = flood_components(c != 0)
    assert n_flood == count and np.array_equal(flood != 0, ids != 0)           # (the flood fill stands in where scipy does not import)
    assert torch.equal(sketch.edges(rgb, 40, 120), ink)


def test_thresholds_and_frames_are_checked():
    from pix2pix3d_amd import sketch
    grey = random_grey(9, 9, seed=1)
    for low, high in ((5, 4), (0, 2041), (-1, 10), (1.5, 10)):
        with pytest.raises(ValueError):
            sketch.edge_classes(grey, low, high)
    with pytest.raises(ValueError):
        sketch.edge_classes(grey.float(), 1, 2)
    with pytest.raises(ValueError):
        sketch.edge_classes(torch.zeros(4, 4, 3, dtype=torch.uint8)[:, :, [2, 1, 0]].permute(1, 0, 2), 1, 2)      # pixels not contiguous


# ---- 4. thinning ---------------------------------------------------------------------------------------------------------------------------
def test_the_deletable_table_is_zhang_suen_and_the_committed_header_is_generated():
    from pix2pix3d_amd import sketch
    table = sketch.deletable_table()
    assert table.dtype == torch.bool and tuple(table.shape) == (2, 256)
    for step in (0, 1):
        for code in range(256):
            assert bool(table[step, code]) == zhang_suen_deletable(step, code), (step, code)
    with open(sketch.THIN_TABLE_PATH) as f:
        assert f.read() == sketch.thin_table_header()


def test_thinning_a_blurred_drawing_reaches_one_pixel_lines_in_two_passes():
    """One-pixel lines, blurred, thresholded at 64: bands three pixels wide.  Two passes reach the fixed point; the lines stay connected and apart."""
    from pix2pix3d_amd import sketch
    ink, n_components = drawing()
    soft = sketch.blur3(ink)
    band = (soft >= 64).to(torch.uint8) * 255
    assert int((band != 0).sum()) > 2 * int((ink != 0).sum())                  # three pixels across the straight lines, fewer across the diagonal
    assert torch.equal(sketch.thin(soft, 64, 0), band)
    results = [sketch.thin(soft, 64, passes) for passes in (1, 2, 3)]
    changes = [int((a != b).sum()) for a, b in zip([band] + results[:-1], results)]
    print('pixels changed per pass', changes, 'left', int((results[1] != 0).sum()), 'drawn', int((ink != 0).sum()))
    assert changes[0] > 0 and changes[2] == 0                                  # a third pass changes nothing
    assert torch.equal(sketch.trace(soft), results[1]) and set(results[1].unique().tolist()) == {0, 255}
    assert label_components(results[1].numpy() != 0)[1] == n_components == label_components(ink.numpy() != 0)[1]
    assert bool(((results[1] != 0) <= (band != 0)).all())                      # thinning only deletes
    on = (results[1] != 0).long()
    four = sum(torch.nn.functional.pad(on, (1, 1, 1, 1))[dy:dy + on.shape[0], dx:dx + on.shape[1]] for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)))
    assert int(four.max()) < 4                                                 # no 2 x 2 block is left: the lines are one pixel wide
    step = sketch.thin_step(soft, 64, 0)
    assert torch.equal(sketch.thin_step(step, 64, 1), results[0])
    for bad in ((0, 0), (256, 0), (64, 2)):
        with pytest.raises(ValueError):
            sketch.thin_step(soft, *bad)


def test_zero_size_images_give_empty_results():
    from pix2pix3d_amd import sketch
    for shape in ((0, 5), (5, 0), (0, 0)):
        empty = torch.zeros(shape, dtype=torch.uint8)
        assert tuple(sketch.blur3(empty).shape) == shape and tuple(sketch.thin(empty).shape) == shape and tuple(sketch.link(empty).shape) == shape
        assert tuple(sketch.edge_classes(empty, 1, 2).shape) == shape and tuple(sketch.edges(torch.zeros(shape + (3,), dtype=torch.uint8), 1, 2).shape) == shape
        assert sketch.condition(empty, 16).numel() == 0
    assert sketch.condition(torch.zeros(4, 4, dtype=torch.uint8), 0).numel() == 0


# ---- 5. a CPU session on a small edge2car generator -----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small_edge_generator():
    return build_generator('edge2car', 'cpu', cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0)


def _session(G, **kwargs):
    from pix2pix3d_amd import sketch
    s = sketch.SketchSession(G, cfg='edge2car', seed=3, neural_rendering_resolution=16, **kwargs)
    ink = torch.zeros(200, 160, dtype=torch.uint8)
    ink[40:160, 80] = 255
    ink[100, 20:140] = 255
    s.load(ink, demo_pose(G))
    return s, ink


@pytest.mark.parametrize('convention', ['dataset', 'input'])
def test_session_encode_equals_mapping_on_the_references_conditioning_image(small_edge_generator, convention):
    from pix2pix3d_amd import edit
    G = small_edge_generator
    s, ink = _session(G, convention=convention, hold_texture=False)
    s.pen([(10, 10, 150, 190, 1)])
    painted = edit.paint_strokes(ink, [(10, 10, 150, 190, 1, 255)]).numpy()
    res = int(G.backbone.mapping.in_resolution)
    want_image = script_condition(numpy_resize_nearest(numpy_blur3(painted), res), convention)
    assert torch.equal(s.condition(), want_image)
    z = torch.from_numpy(np.random.RandomState(3).randn(1, G.z_dim).astype('float32'))
    pose = torch.from_numpy(demo_pose(G))[None]
    with torch.no_grad():
        want = G.mapping(z, edit.forward_label(G), {'mask': want_image, 'pose': pose})
    assert torch.equal(s.encode(), want)
    frame = s.frame()
    r = G.img_resolution
    assert frame['image'].shape == (r, r, 3) and frame['label'].shape == (r, r) and frame['image'].dtype == frame['label'].dtype == np.uint8


def test_session_pen_erase_undo_and_clear_round_trip_the_canvas(small_edge_generator, tmp_path):
    from pix2pix3d_amd import edit
    s, ink = _session(small_edge_generator)
    assert s.canvas is s._base and torch.equal(s.canvas, ink)
    s.pen([(5, 5, 100, 60, 3), (100, 60, 150, 20, 1)])
    penned = edit.paint_strokes(ink, [(5, 5, 100, 60, 3, 255), (100, 60, 150, 20, 1, 255)])
    assert torch.equal(s.canvas, penned) and not torch.equal(penned, ink)
    s.erase([(80, 0, 80, 199, 9)])
    erased = edit.paint_strokes(penned, [(80, 0, 80, 199, 9, 0)])
    assert torch.equal(s.canvas, erased) and int(erased[:, 80].max()) == 0 and len(s.log) == 2
    s.undo()
    assert torch.equal(s.canvas, penned)
    s.erase([(80, 0, 80, 199, 9)])
    s.clear()
    assert torch.equal(s.canvas, ink) and len(s.log) == 0
    s.undo()
    assert torch.equal(s.canvas, ink)
    for bad in ([(1, 2, 3, 4)], [(1, 2, 3, 4, 0)], [(1, 2, 3, 4, 5, 255)], [(1.5, 2, 3, 4, 5)]):
        with pytest.raises(ValueError):
            s.pen(bad)
    s.pen([(5, 5, 100, 60, 3)])
    s.save(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ['canvas.png', 'condition.png', 'output.png']


def test_session_undo_and_clear_followed_by_strokes_without_a_read_in_between(small_edge_generator):
    """The kept canvas must never serve as the prefix of a log it is ahead of: every sequence below appends after ``undo`` / ``clear`` BEFORE the canvas is read again."""
    from pix2pix3d_amd import edit
    a, b, c, d = (10, 20, 150, 20, 1), (10, 60, 150, 60, 3), (10, 120, 150, 120, 1), (30, 5, 30, 190, 5)

    def painted(ink, rows):
        return edit.paint_strokes(ink, [r + (255,) for r in rows]) if rows else ink

    s, ink = _session(small_edge_generator)
    s.pen([a]); s.pen([b])
    assert torch.equal(s.canvas, painted(ink, [a, b]))
    s.undo(); s.pen([c])                                                       # b is gone, c is new: the kept canvas of [a, b] is no prefix of [a, c]
    assert torch.equal(s.canvas, painted(ink, [a, c])) and int(s.canvas[60, 30]) == 0
    assert torch.equal(s.condition(), sketch_condition(painted(ink, [a, c]), small_edge_generator))
    s.clear(); s.pen([d]); s.pen([b])
    assert torch.equal(s.canvas, painted(ink, [d, b]))
    s.undo(); s.undo(); s.pen([c]); s.pen([a]); s.pen([d])
    assert torch.equal(s.canvas, painted(ink, [c, a, d]))
    s.pen([b]); s.undo()                                                       # an entry that was never read: the kept canvas of [c, a, d] still is a prefix
    kept = s._kept
    s.pen([b])
    assert s._kept is kept and torch.equal(s.canvas, painted(ink, [c, a, d, b]))
    s.undo(); s.undo(); s.undo(); s.undo(); s.undo()
    assert s.canvas is s._base and torch.equal(s.canvas, ink)


def sketch_condition(canvas, G):
    from pix2pix3d_amd import sketch
    return sketch.condition(canvas, int(G.backbone.mapping.in_resolution))


def test_results_must_not_share_bytes_with_their_inputs():
    from pix2pix3d_amd import sketch
    store = torch.zeros(40, 40, dtype=torch.uint8)
    image = store[2:22, 2:22]
    for out in (image, store[3:23, 3:23], store[10:30, 0:20]):                 # the input itself, a shifted window, a window whose rows interleave with it
        for call in (lambda: sketch.thin_step(image, 64, 0, out=out), lambda: sketch.edge_classes(image, 1, 2, out=out), lambda: sketch.link(image, out=out)):
            with pytest.raises(ValueError):
                call()
    assert torch.equal(sketch.thin_step(image, 64, 0, out=torch.zeros(45, 25, dtype=torch.uint8)[25:45, 2:22]), sketch.thin_step(image, 64, 0))      # another store
    below = store[22:40, 0:20]                                                 # wholly after the input's rows in the same store: allowed
    assert torch.equal(sketch.thin_step(store[2:20, 2:22], 64, 0, out=below), sketch.thin_step(store[2:20, 2:22].clone(), 64, 0))


def test_sessions_name_their_own_load_when_nothing_is_loaded(small_edge_generator):
    from pix2pix3d_amd import edit, sketch
    with pytest.raises(RuntimeError, match=r'SketchSession: load\(ink, pose\) first'):
        sketch.SketchSession(small_edge_generator).pen([(1, 1, 2, 2, 1)])
    seg = build_generator('seg2cat', 'cpu', cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0)
    with pytest.raises(RuntimeError, match=r'EditSession: load\(mask, pose\) first'):
        edit.EditSession(seg).mask


def test_session_camera_moves_keep_the_ws_and_the_view_comes_back_as_a_canvas(small_edge_generator):
    from pix2pix3d_amd import sketch
    G = small_edge_generator
    s, ink = _session(G)
    first, ws = s.render(), s.encode()
    s.set_camera(yaw=30, pitch=50)
    turned = s.render()
    assert s.encode() is ws and not torch.equal(turned['image'], first['image'])
    s.take_view_as_canvas()
    assert torch.equal(s.canvas, sketch.trace(255 - turned['label'])) and len(s.log) == 0 and set(s.canvas.unique().tolist()) <= {0, 255}
    assert s.encode() is not ws
    s.load_image(scene(), demo_pose(G), 40, 120)
    assert torch.equal(s.canvas, sketch.edges(scene(), 40, 120))


def test_each_session_refuses_the_other_kind_of_generator(small_edge_generator):
    from pix2pix3d_amd import edit, sketch
    seg = build_generator('seg2cat', 'cpu', cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0)
    with pytest.raises(TypeError):
        sketch.SketchSession(seg)
    with pytest.raises(TypeError):
        edit.EditSession(small_edge_generator, cfg='edge2car')
    with pytest.raises(ValueError):
        sketch.SketchSession(small_edge_generator, convention='files')
    with pytest.raises(RuntimeError):
        sketch.SketchSession(small_edge_generator).canvas
