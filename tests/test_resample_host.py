"""pix2pix3d_amd.resample on the host: the CPU formulation (the definition) against ``PIL.Image.resize`` byte for byte — live, and from a golden recorded
with Pillow 12.2.0 —, the arithmetic of the coefficient tables, and the contract: every argument error before the library is touched, where the
prototypes sit in the header, and the new keyword arguments at their defaults."""
import json
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from resample_cases import (BOXES, MODES, NEAREST_PAIRS, SEPARABLE, SIZE_PAIRS, binary_clip, label_clip, pil_resize, uniform_clip)

from pix2pix3d_amd import resample


def _recorded_pillow():
    return str(load_golden('resample_pil')['pillow'])


def _live_pil():
    """Skip (not fail) the live comparison under another Pillow than the recorded one: the golden comparison below pins the same bytes and never skips."""
    import PIL
    if PIL.__version__ != _recorded_pillow():
        pytest.skip(f'Pillow {PIL.__version__} is installed, the golden was recorded with {_recorded_pillow()}')


def _clip(h, w, bpp, seed, binary):
    return (binary_clip if binary else uniform_clip)(1, h, w, bpp, seed=seed)


# ---- PIL equality ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('filter', SEPARABLE)
@pytest.mark.parametrize('mode', list(MODES))
def test_the_cpu_formulation_equals_pil_at_every_size_pair(mode, filter):
    _live_pil()
    for n, ((w, h), size) in enumerate(SIZE_PAIRS):
        for binary in (False, True):
            clip = _clip(h, w, MODES[mode], 10 * n + binary, binary)
            assert torch.equal(resample.resize(clip, size, filter)[0], pil_resize(clip[0], mode, size, filter)), (mode, filter, (w, h), size, binary)


@pytest.mark.parametrize('filter', SEPARABLE)
def test_the_cpu_formulation_equals_pil_with_a_box(filter):
    _live_pil()
    for n, ((w, h), box, size) in enumerate(BOXES):
        for mode in ('L', 'RGB'):
            clip = _clip(h, w, MODES[mode], 50 + n, binary=n % 2 == 1)
            assert torch.equal(resample.resize(clip, size, filter, box=box)[0], pil_resize(clip[0], mode, size, filter, box)), (mode, filter, box)


def test_nearest_equals_pil_where_the_closed_form_does_not():
    _live_pil()
    for n, ((w, h), size) in enumerate(NEAREST_PAIRS):
        clip = uniform_clip(1, h, w, 1, seed=70 + n)
        assert torch.equal(resample.resize(clip, size, 'nearest')[0], pil_resize(clip[0], 'L', size, 'nearest')), ((w, h), size)
    closed = torch.tensor([int((x + 0.5) * 512 / 300) for x in range(300)], dtype=torch.int32)
    assert not torch.equal(closed, resample.nearest_indices(512, 300))                     # the accumulated table is another table


def test_the_golden_pins_pils_bytes():
    golden = load_golden('resample_pil')
    asked = json.loads(str(golden['asked']))
    assert len(asked) >= 30 and {a['filter'] for a in asked.values()} == set(resample.FILTERS)
    for name, a in asked.items():
        frame = torch.from_numpy(golden[f'in_{name}'])
        got = resample.resize(frame[None], tuple(a['size']), a['filter'], box=None if a['box'] is None else tuple(a['box']))[0]
        assert torch.equal(got, torch.from_numpy(golden[f'out_{name}'])), name


# ---- arithmetic -------------------------------------------------------------------------------------------------------------------------------
SUPPORT = {'box': 0.5, 'bilinear': 1.0, 'hamming': 1.0, 'bicubic': 2.0, 'lanczos': 3.0}


@pytest.mark.parametrize('filter', SEPARABLE)
def test_tables_sum_to_one_stay_inside_the_axis_and_have_the_formulas_ksize(filter):
    for in_size, out_size, interval in ((17, 5, None), (17, 40, None), (512, 1, None), (8, 64, None), (50, 49, None), (50, 20, (3.5, 41.0)), (33, 33, (0.5, 32.5)),
                                        (1, 64, None)):
        bounds, weights = resample.coefficients(in_size, out_size, filter, interval)
        in0, in1 = interval or (0.0, float(in_size))
        ksize = int(math.ceil(SUPPORT[filter] * max((in1 - in0) / out_size, 1.0))) * 2 + 1
        assert bounds.dtype == weights.dtype == torch.int32 and tuple(bounds.shape) == (out_size, 2) and tuple(weights.shape) == (out_size, ksize)
        xmin, count = bounds[:, 0], bounds[:, 1]
        assert bool((xmin >= 0).all()) and bool((count >= 1).all()) and bool((xmin + count <= in_size).all()) and bool((count <= ksize).all())
        live = torch.arange(ksize)[None] < count[:, None]
        assert bool((weights[~live] == 0).all())
        # every entry is rounded to the nearest 2^-22 (half a unit each), and the floats they were rounded from sum to one within their own rounding
        assert bool(((weights.sum(1) - (1 << 22)).abs() <= count / 2 + 1).all()), (filter, in_size, out_size)


def test_the_int32_bound_raises_on_a_fabricated_table():
    resample.check_weights(torch.full([2, 2], 1 << 22, dtype=torch.int32))
    worst = ((1 << 31) - (1 << 21)) // 255                                                # the largest sum of |k| that still fits
    resample.check_weights(torch.tensor([[worst, 0], [-(worst // 2), worst - worst // 2 - 1]], dtype=torch.int32))
    with pytest.raises(ValueError, match='2\\^31'):
        resample.check_weights(torch.tensor([[worst // 2 + 1, -(worst - worst // 2)]], dtype=torch.int32))


def test_two_channel_clips_equal_two_grey_resizes():
    clip = binary_clip(2, 23, 17, 2, seed=5)
    for filter in SEPARABLE + ('nearest',):
        for size in ((5, 7), (40, 31)):
            got = resample.resize(clip, size, filter)
            for c in range(2):
                assert torch.equal(got[..., c], resample.resize(clip[..., c].contiguous(), size, filter)), (filter, size, c)


def test_the_unclamped_sums_of_binary_noise_leave_the_byte_range():
    clip = binary_clip(1, 8, 8, 1, seed=300)
    for filter in ('bicubic', 'lanczos'):
        sums = resample.pass_sums(clip, 2, *resample.coefficients(8, 64, filter)) >> resample.PRECISION_BITS
        assert int(sums.min()) < 0 and int(sums.max()) > 255
        out = resample.resize(clip, 64, filter)
        assert int(out.min()) == 0 and int(out.max()) == 255


def test_the_passes_skip_what_they_may_and_pitched_views_are_taken():
    clip = uniform_clip(3, 20, 33, 3, seed=9)
    same = resample.resize(clip, (33, 20), 'lanczos')
    assert torch.equal(same, clip) and same.data_ptr() != clip.data_ptr()                   # both axes skipped: a copy
    canvas = torch.zeros([5, 40, 50, 3], dtype=torch.uint8)
    out = canvas[1:4, 3:12, 5:38]
    assert resample.resize(clip, (33, 9), 'bicubic', out=out) is out and torch.equal(out, resample.resize(clip, (33, 9), 'bicubic'))
    assert int(canvas.sum()) == int(out.long().sum())                                       # nothing written beside the view
    view = torch.from_numpy(np.random.default_rng(4).integers(0, 256, size=(6, 64, 96, 3), dtype=np.uint8))[::2, 9:54, 11:88]
    assert torch.equal(resample.resize(view, (20, 31), 'hamming'), resample.resize(view.contiguous(), (20, 31), 'hamming'))
    empty = resample.resize(clip[:0], (7, 5), 'box')
    assert tuple(empty.shape) == (0, 5, 7, 3) and empty.dtype == torch.uint8
    assert torch.equal(resample.thumbnails(clip, 8), resample.resize(clip, (8, 8), 'lanczos'))
    labels = label_clip(2, 23, 17, seed=3)
    for size in ((5, 7), (40, 31)):
        assert set(resample.resize(labels, size, 'nearest').unique().tolist()) <= set(labels.unique().tolist())


def test_the_table_cache_is_bounded_and_counts():
    resample.cache_clear()
    clip = uniform_clip(1, 20, 33, 1, seed=1)
    resample.resize(clip, (9, 7), 'bilinear')
    first = resample.cache_info()
    assert first['builds'] == 2 and first['hits'] == 0
    resample.resize(clip, (9, 7), 'bilinear')
    assert resample.cache_info() == dict(first, hits=2)
    for n in range(1, resample.CACHE_ENTRIES + 8):
        resample.resize(clip, (n, 20), 'box')
    assert resample.cache_info()['entries'] == resample.CACHE_ENTRIES


# ---- contract ---------------------------------------------------------------------------------------------------------------------------------
def test_every_argument_error_is_a_valueerror_before_the_library_is_touched(monkeypatch):
    from pix2pix3d_amd import clips

    def touched():
        raise AssertionError('the library was touched')
    monkeypatch.setattr(clips, 'video_lib', touched)
    monkeypatch.setattr(clips._side, 'lib', touched)
    clip = uniform_clip(2, 20, 33, 3, seed=2)
    bad = [lambda: resample.resize(clip, (5, 5), 'cubic'),                                  # unknown filter
           lambda: resample.resize(clip, (5, 5), 'box', box=(4.0, 2.0, 4.0, 9.0)),          # empty box
           lambda: resample.resize(clip, (5, 5), 'box', box=(9.0, 2.0, 4.0, 9.0)),          # inverted box
           lambda: resample.resize(clip, (5, 5), 'box', box=(0.0, 0.0, 33.5, 20.0)),        # box outside the image
           lambda: resample.resize(clip, (5, 5), 'box', box=(-0.5, 0.0, 33.0, 20.0)),
           lambda: resample.resize(clip, (5, 5), 'nearest', box=(0.0, 0.0, 4.0, 9.0)),      # nearest takes no box
           lambda: resample.resize(clip.float(), (5, 5)),                                   # not uint8
           lambda: resample.resize(clip[0, 0], (5, 5)),                                     # wrong rank
           lambda: resample.resize(clip[..., None], (5, 5)),
           lambda: resample.resize(torch.zeros([1, 4, 4, 5], dtype=torch.uint8), (5, 5)),   # five bytes a pixel
           lambda: resample.resize(clip, (5, 0)), lambda: resample.resize(clip, (5, 5, 5)), lambda: resample.resize(clip, 2.5),
           lambda: resample.resize(clip, (5, 5), out=torch.empty([2, 5, 6, 3], dtype=torch.uint8)),      # out of the wrong shape
           lambda: resample.resize(clip, (5, 5), out=torch.empty([2, 5, 5, 3], dtype=torch.int16)),
           lambda: resample.resize(clip, (5, 5), out=torch.empty([2, 5, 5, 3], dtype=torch.uint8, device='meta')),      # out on another device
           lambda: resample.resize(clip, (33, 20), out=clip),                               # in place
           lambda: resample.coefficients(8, 4, 'nearest'), lambda: resample.coefficients(8, 0, 'box'), lambda: resample.coefficients(8, 4, 'box', (3.0, 9.0)),
           lambda: resample.nearest_indices(0, 4)]
    for n, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f'case {n} raised nothing')
    assert resample.FILTERS == ('nearest', 'box', 'bilinear', 'hamming', 'bicubic', 'lanczos')


def test_the_prototypes_are_the_video_headers_alone_and_the_product_abi_gains_nothing():
    from pix2pix3d_amd import _lib, clips, decimate, sketch
    names = ['p3d_frame_resample_rows', 'p3d_frame_resample_columns', 'p3d_frame_resample_nearest']
    assert all(n in clips.HEADER.functions for n in names)
    assert not any(n in header.functions for n in names for header in (_lib.HEADER, sketch.HEADER, decimate.HEADER))
    assert set(sketch.HEADER.functions) == {'p3d_sketch_condition', 'p3d_sketch_edge_classes', 'p3d_sketch_link', 'p3d_sketch_thin_step'}
    assert (resample.TILE_W, resample.TILE_H) == (clips.HEADER.constants['P3D_RESAMPLE_TILE_W'], clips.HEADER.constants['P3D_RESAMPLE_TILE_H'])


def test_the_new_keywords_at_their_defaults_change_no_byte(tmp_path):
    from PIL import Image
    from model_cases import build_generator
    from pix2pix3d_amd import edit, sketch, views
    G = build_generator('seg2cat', 'cpu', cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0)
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(8))
    kw = dict(n_frames=2, views_per_step=2, neural_rendering_resolution=16)
    files = {}
    for tag, extra in (('omitted', {}), ('defaults', dict(size=None, resample='lanczos'))):
        torch.manual_seed(3)
        out = views.generate_video(G, ws, 'seg2cat', str(tmp_path / f'{tag}_v.gif'), str(tmp_path / f'{tag}_l.gif'), **kw, **extra)
        files[tag] = ((tmp_path / f'{tag}_v.gif').read_bytes(), (tmp_path / f'{tag}_l.gif').read_bytes(), out)
    assert files['omitted'][:2] == files['defaults'][:2]
    assert all(torch.equal(files['omitted'][2][k], files['defaults'][2][k]) for k in ('image', 'label', 'label_index'))
    torch.manual_seed(3)
    small = views.generate_video(G, ws, 'seg2cat', size=(24, 20), resample='bicubic', **kw)       # and with a size: the resize of those frames
    full = files['omitted'][2]
    assert torch.equal(small['image'], resample.resize(full['image'], (24, 20), 'bicubic'))
    assert torch.equal(small['label'], resample.resize(full['label'], (24, 20), 'nearest'))
    assert torch.equal(small['label_index'], resample.resize(full['label_index'], (24, 20), 'nearest'))
    with pytest.raises(ValueError):
        views.generate_video(G, ws, 'seg2cat', size=24, resample='cubic', **kw)
    camera, shots = views.video_cameras(G, 'seg2cat', 2)[0], []
    for extra in ({}, dict(size=None, resample='lanczos'), dict(size=(12, 10), resample='box')):
        torch.manual_seed(3)
        shots.append(views.generate_sample(G, ws, camera, str(tmp_path / f'c{len(shots)}.png'), neural_rendering_resolution=16, **extra))
    assert (tmp_path / 'c0.png').read_bytes() == (tmp_path / 'c1.png').read_bytes() and torch.equal(shots[0]['image'], shots[1]['image'])
    assert torch.equal(shots[2]['image'], resample.resize(shots[0]['image'], (12, 10), 'box'))
    assert torch.equal(shots[2]['label_index'], resample.resize(shots[0]['label_index'], (12, 10), 'nearest'))
    with Image.open(tmp_path / 'c2.png') as im:
        assert np.array_equal(np.asarray(im), shots[2]['image'][0].numpy())
    frames = uniform_clip(6, 10, 12, 3, seed=6)
    assert torch.equal(views.image_grid(frames, (3, 2), cell=None), views.image_grid(frames, (3, 2)))
    assert torch.equal(views.image_grid(frames, (3, 2), cell=(6, 5)), views.image_grid(resample.resize(frames, (6, 5)), (3, 2)))
    mask = label_clip(1, 24, 16, seed=7)[0]
    Image.fromarray(mask.numpy()).save(tmp_path / 'mask.png')
    assert torch.equal(edit.load_mask(str(tmp_path / 'mask.png'), 'cpu', size=None), edit.load_mask(str(tmp_path / 'mask.png'), 'cpu'))
    assert torch.equal(edit.load_mask(str(tmp_path / 'mask.png'), 'cpu'), mask)
    assert torch.equal(edit.load_mask(str(tmp_path / 'mask.png'), 'cpu', size=(8, 12)), resample.resize(mask[None], (8, 12), 'nearest')[0])
    assert torch.equal(sketch.load_canvas(str(tmp_path / 'mask.png'), 'cpu', size=None, filter='box'), sketch.load_canvas(str(tmp_path / 'mask.png'), 'cpu'))
    assert torch.equal(sketch.load_canvas(str(tmp_path / 'mask.png'), 'cpu', size=(8, 12)), resample.resize(mask[None], (8, 12), 'box')[0])
