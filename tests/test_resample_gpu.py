"""pix2pix3d_amd.resample on the device: the bytes of p3d_frame_resample_rows, p3d_frame_resample_columns and p3d_frame_resample_nearest against the CPU
formulation on the host copy (integer equality) and the launch counts resample.py states, at the smallest shapes that can go wrong: a pitched, offset,
frame-strided window with 1 .. 4 bytes a pixel into a pitched ``out=``; outputs around one work-group tile for both passes; tap lists too long for LDS
(512 -> 1, both axes); one source pixel; outputs whose every tap list is clipped at a border; noise that reaches both clamps; boxes; labels; offsets
past 2^31; the table cache; and the writers and loaders that take a size."""
import warnings

import numpy as np
import pytest
import torch

from resample_cases import BOXES, SEPARABLE, binary_clip, label_clip, uniform_clip

pytestmark = pytest.mark.gpu


def _agrees(clip, size, filter, box=None, pitched=True):
    """resize on the device — into a pitched window of a canvas whose other bytes must survive — equals resize on the host copy."""
    from pix2pix3d_amd import resample
    expected = resample.resize(clip.cpu(), size, filter, box=box)
    if not pitched:
        got = resample.resize(clip, size, filter, box=box)
        assert got.is_cuda and torch.equal(got.cpu(), expected), (tuple(clip.shape), size, filter, box)
        return got
    f, oh, ow = expected.shape[:3]
    canvas = torch.full([f + 1, oh + 3, ow + 5] + list(expected.shape[3:]), 0xA5, dtype=torch.uint8, device='cuda')
    out = canvas[1:, 1:1 + oh, 2:2 + ow]
    assert resample.resize(clip, size, filter, box=box, out=out) is out
    assert torch.equal(out.cpu(), expected), (tuple(clip.shape), size, filter, box)
    out.fill_(0xA5)
    assert bool((canvas == 0xA5).all()), 'a store left the window'
    return expected


@pytest.mark.parametrize('bpp', [1, 2, 3, 4])
def test_a_strided_window_into_a_pitched_out(hip_lib, bpp):
    canvas = uniform_clip(6, 64, 96, bpp, seed=20 + bpp).cuda()
    view = canvas[::2, 9:54, 11:88]
    assert not view.is_contiguous() and view.storage_offset() == (9 * 96 + 11) * bpp and view.stride(0) == 2 * 64 * 96 * bpp
    for filter in SEPARABLE:
        _agrees(view, (20, 31), filter)
        _agrees(view, (100, 150), filter)


def test_outputs_around_one_tile_for_both_passes(hip_lib):
    from pix2pix3d_amd import resample
    tw, th = resample.TILE_W, resample.TILE_H
    rgbx, grey = uniform_clip(2, 24, 80, 4, seed=30).cuda(), uniform_clip(2, 40, 4 * tw + 1, 1, seed=31).cuda()
    for dw in (-1, 0, 1):
        for dh in (-1, 0, 1):
            _agrees(rgbx, (tw + dw, th + dh), 'bicubic')                                  # rows: tw + dw pixels of 24 rows; columns: (tw + dw) dwords, th + dh rows
        rows = uniform_clip(2, th + dw, 40, 3, seed=32 + dw).cuda()
        for ow in (tw - 1, tw, tw + 1):
            _agrees(rows, (ow, th + dw), 'bilinear')                                       # the horizontal pass alone, th + dw rows
        for w in (4 * tw - 1, 4 * tw, 4 * tw + 1):                                         # the vertical pass alone: a row of one tile of dwords, and a byte either way
            _agrees(grey[:, :, :w], (w, th + dw), 'hamming')


def test_tap_lists_too_long_for_lds_on_both_axes(hip_lib):
    from pix2pix3d_amd import resample
    assert resample.coefficients(512, 1, 'lanczos')[1].shape[1] == 3073
    _agrees(uniform_clip(2, 3, 512, 3, seed=40).cuda(), (1, 3), 'lanczos')
    _agrees(uniform_clip(2, 512, 3, 3, seed=41).cuda(), (3, 1), 'lanczos')
    _agrees(uniform_clip(1, 20, 512, 1, seed=42).cuda(), (40, 20), 'lanczos')             # 79 taps: more than the LDS table holds
    _agrees(uniform_clip(1, 5, 2100, 1, seed=43).cuda(), (100, 5), 'box')                 # 23 taps, but a tile's span is 1344 bytes: more than an LDS row holds


def test_one_source_pixel_and_outputs_clipped_at_both_borders(hip_lib):
    for filter in SEPARABLE:
        _agrees(uniform_clip(2, 1, 1, 3, seed=50).cuda(), (64, 64), filter)                # count is 1 everywhere
        for size in ((2, 3), (3, 2)):
            _agrees(uniform_clip(2, 23, 17, 3, seed=51).cuda(), size, filter)
            _agrees(uniform_clip(2, 2, 3, 1, seed=52).cuda(), size, filter)


def test_binary_noise_reaches_both_clamps(hip_lib):
    from pix2pix3d_amd import resample
    clip = binary_clip(1, 8, 8, 1, seed=300)
    for filter in ('bicubic', 'lanczos'):
        sums = resample.pass_sums(clip, 2, *resample.coefficients(8, 64, filter)) >> resample.PRECISION_BITS
        assert int(sums.min()) < 0 and int(sums.max()) > 255                               # the unclamped sums of the CPU formulation leave [0, 255]
        out = _agrees(clip.cuda(), (64, 64), filter, pitched=False)
        assert int(out.min()) == 0 and int(out.max()) == 255


def test_launch_counts(hip_lib):
    from pix2pix3d_amd import clips, resample
    clip = uniform_clip(2, 20, 33, 3, seed=60).cuda()

    def launches(fn):
        n0 = clips.launch_count()
        out = fn()
        return clips.launch_count() - n0, out
    assert launches(lambda: _agrees(clip, (33, 9), 'lanczos', pitched=False))[0] == 1      # a single axis
    assert launches(lambda: _agrees(clip, (12, 20), 'lanczos', pitched=False))[0] == 1
    assert launches(lambda: _agrees(clip, (12, 9), 'lanczos', pitched=False))[0] == 2      # both
    assert launches(lambda: _agrees(clip, (12, 9), 'nearest', pitched=False))[0] == 1
    n, same = launches(lambda: resample.resize(clip, (33, 20), 'bicubic'))
    assert n == 0 and torch.equal(same, clip) and same.data_ptr() != clip.data_ptr()       # a copy_
    n, empty = launches(lambda: resample.resize(clip[:0], (12, 9), 'bicubic'))
    assert n == 0 and tuple(empty.shape) == (0, 9, 12, 3) and empty.is_cuda and empty.dtype == torch.uint8
    n, empty = launches(lambda: resample.resize(clip[:0], (12, 9), 'nearest'))
    assert n == 0 and tuple(empty.shape) == (0, 9, 12, 3)


def test_boxes(hip_lib):
    for n, ((w, h), box, size) in enumerate(BOXES):
        clip = uniform_clip(2, h, w, 3, seed=70 + n).cuda()
        for filter in SEPARABLE:
            _agrees(clip, size, filter, box=box)


def test_nearest_keeps_every_label(hip_lib):
    labels = label_clip(2, 45, 77, seed=80)
    canvas = torch.zeros([2, 50, 90], dtype=torch.uint8)
    canvas[:, 3:48, 5:82] = labels
    view = canvas.cuda()[:, 3:48, 5:82]
    for size in ((20, 31), (100, 150), (300, 45)):
        out = _agrees(view, size, 'nearest')
        assert set(out.unique().tolist()) <= set(labels.unique().tolist())
    _agrees(uniform_clip(2, 23, 17, 3, seed=81).cuda(), (40, 7), 'nearest')


def test_offsets_past_2_31(hip_lib):
    """Three 8 x 8 x 3 frames 2^30 bytes apart over one uninitialised allocation of 2^31 + 192 bytes — the smallest they fit in —, frame 2 at byte 2^31."""
    store = torch.empty([(1 << 31) + 192], dtype=torch.uint8, device='cuda')
    clip = store.as_strided([3, 8, 8, 3], [1 << 30, 24, 3, 1])
    host = uniform_clip(3, 8, 8, 3, seed=90)
    clip.copy_(host)                                                                       # only the three frames are written
    assert clip.data_ptr() + 2 * clip.stride(0) == store.data_ptr() + (1 << 31)
    for size, filter in (((5, 5), 'lanczos'), ((5, 8), 'bilinear'), ((8, 5), 'bilinear'), ((5, 5), 'nearest')):      # both passes, each alone, the gather
        _agrees(clip, size, filter, pitched=False)


def test_a_repeated_call_uploads_nothing_and_never_synchronises(hip_lib):
    from pix2pix3d_amd import resample
    clip = uniform_clip(2, 20, 33, 3, seed=95).cuda()
    resample.resize(clip, (12, 9), 'lanczos')
    resample.resize(clip, (12, 9), 'nearest')
    torch.cuda.synchronize()
    before = resample.cache_info()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            a, b = resample.resize(clip, (12, 9), 'lanczos'), resample.resize(clip, (12, 9), 'nearest')
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    assert [str(w.message) for w in caught if 'called a synchronizing' in str(w.message)] == []
    after = resample.cache_info()
    assert after['builds'] == before['builds'] and after['hits'] == before['hits'] + 4      # two tables a call, none made
    assert torch.equal(a.cpu(), resample.resize(clip.cpu(), (12, 9), 'lanczos')) and torch.equal(b.cpu(), resample.resize(clip.cpu(), (12, 9), 'nearest'))


def test_generate_video_and_load_mask_take_a_size(hip_lib, tmp_path):
    from PIL import Image
    from model_cases import build_generator
    from png_cases import decode_apng
    from pix2pix3d_amd import edit, resample, views
    G = build_generator('seg2cat', 'cuda', depth=(64, 64))
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(41)).cuda()
    kw = dict(n_frames=4, views_per_step=4, jitter='frozen')
    torch.manual_seed(5)
    full = views.generate_video(G, ws, 'seg2cat', **kw)
    torch.manual_seed(5)
    out = views.generate_video(G, ws, 'seg2cat', str(tmp_path / 'v.png'), str(tmp_path / 'l.png'), size=64, format='apng', **kw)
    assert tuple(out['image'].shape) == (4, 64, 64, 3) and out['image'].is_cuda
    assert torch.equal(out['image'], resample.resize(full['image'], 64, 'lanczos'))
    assert torch.equal(out['label'], resample.resize(full['label'], 64, 'nearest'))
    assert torch.equal(out['label_index'], resample.resize(full['label_index'], 64, 'nearest'))
    got, _, _ = decode_apng(tmp_path / 'v.png')
    assert all(np.array_equal(g, f.cpu().numpy()) for g, f in zip(got, out['image']))
    with Image.open(tmp_path / 'l.png') as im:
        assert im.n_frames == 4
        for i in range(4):
            im.seek(i)
            assert np.array_equal(np.asarray(im.convert('RGB')), out['label'][i].cpu().numpy())
    mask = label_clip(1, 96, 128, seed=7)[0]
    Image.fromarray(mask.numpy()).save(tmp_path / 'mask.png')
    loaded = edit.load_mask(str(tmp_path / 'mask.png'), 'cuda')
    sized = edit.load_mask(str(tmp_path / 'mask.png'), 'cuda', size=(64, 48))
    assert sized.is_cuda and torch.equal(sized, resample.resize(loaded[None], (64, 48), 'nearest')[0])
    assert torch.equal(sized.cpu(), resample.resize(mask[None], (64, 48), 'nearest')[0])
