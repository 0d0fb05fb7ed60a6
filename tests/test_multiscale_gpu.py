"""pix2pix3d_amd.multiscale on the device: the sums of p3d_frame_msssim_level and the levels of p3d_frame_halve and of the fused launch against the CPU
formulation on the host copy — ``torch.equal``, no tolerance — and the launch counts multiscale.py states, at the smallest shapes that can go wrong: five
levels with odd sizes at three of them and a single window at the last; more pixel tiles than window tiles both ways; one window past a tile edge each
way; pitched, offset, frame-strided views read in place; both routes; accumulation without a synchronisation; no frame; and the ``ms_ssim=`` target of
``jpeg_quality_for``."""
import warnings

import numpy as np
import pytest
import torch

from multiscale_cases import SINGLE_LEVEL_SIZES, pairs, single_level_agrees
from quality_cases import checkerboard, clip, disturbed, in_canvas

pytestmark = pytest.mark.gpu


def _m():
    from pix2pix3d_amd import multiscale
    return multiscale


def _launches(fn):
    from pix2pix3d_amd import clips
    n0 = clips.launch_count()
    out = fn()
    return clips.launch_count() - n0, out


def _agrees(a, b, levels):
    """Both routes on the device equal the CPU formulation on the host copies; returns the sums."""
    M = _m()
    expected = M.msssim_sums(a.cpu(), b.cpu(), levels)
    n_fused, fused = _launches(lambda: M.msssim_sums(a, b, levels))
    n_split, split = _launches(lambda: M.msssim_sums(a, b, levels, fused=False))
    assert fused.is_cuda and fused.dtype == torch.int64 and torch.equal(fused.cpu(), expected), (tuple(a.shape), levels, 'fused')
    assert torch.equal(split.cpu(), expected), (tuple(a.shape), levels, 'fused=False')
    assert (n_fused, n_split) == (levels, 3 * levels - 2)
    return expected


def _levels_agree(a, b, levels):
    """The levels the fused launch writes — into the caller's buffers, through the entry point — equal ``halve``'s on the device and on the host."""
    M = _m()
    host_a, host_b = M.pyramid(a.cpu(), levels), M.pyramid(b.cpu(), levels)
    sums = torch.zeros([a.shape[0], a.shape[3] if a.ndim == 4 else 1, levels, 3], dtype=torch.int64, device='cuda')
    for k in range(levels - 1):
        shape = [a.shape[0], a.shape[1] // 2, a.shape[2] // 2] + list(a.shape[3:])
        guard = [torch.full([int(np.prod(shape)) + 64], 0xA5, dtype=torch.uint8, device='cuda') for _ in range(2)]      # 32 bytes either side of a level
        next_a, next_b = (g[32:-32].view(shape) for g in guard)
        M.level_sums(a, b, sums, k, next_a, next_b)
        assert torch.equal(next_a.cpu(), host_a[k + 1]) and torch.equal(next_b.cpu(), host_b[k + 1]), (k, tuple(a.shape))
        assert torch.equal(M.halve(a), next_a) and torch.equal(M.halve(b), next_b)
        assert all(bool((g[:32] == 0xA5).all()) and bool((g[-32:] == 0xA5).all()) for g in guard), 'a store left the level'
        a, b = next_a, next_b
    M.level_sums(a, b, sums, levels - 1)
    return sums


def test_five_levels_with_odd_sizes_and_a_single_window_at_the_last(hip_lib):
    M = _m()
    a = clip(2, 177, 190, 3, seed=101)
    b = disturbed(a, seed=102)
    assert [tuple(t.shape[1:3]) for t in M.pyramid(a)] == [(177, 190), (88, 95), (44, 47), (22, 23), (11, 11)]
    expected = _agrees(a.cuda(), b.cuda(), 5)
    assert expected[0, 0, :, 2].tolist() == [167 * 180, 78 * 85, 34 * 37, 12 * 13, 1]
    assert torch.equal(_levels_agree(a.cuda(), b.cuda(), 5).cpu(), expected)
    assert M.ms_ssim(a.cuda(), b.cuda()) == M.ms_ssim(a, b)


@pytest.mark.parametrize('bpp', [1, 2, 3, 4])
def test_more_pixel_tiles_than_window_tiles_both_ways(hip_lib, bpp):
    """2 x 2 tiles of windows, 3 x 3 tiles of pixels: the work-groups of the last row and column own no window and still write the next level."""
    M = _m()
    h, w = 2 * M.TILE_H + 10, 2 * M.TILE_W + 10                                   # 42 x 74 with the 32 x 16 tile
    assert -(-h // M.TILE_H) == 3 > -(-(h - 10) // M.TILE_H) and -(-w // M.TILE_W) == 3 > -(-(w - 10) // M.TILE_W)
    a = clip(3, h, w, bpp, seed=110 + bpp)
    b = disturbed(a, seed=120 + bpp)
    expected = _agrees(a.cuda(), b.cuda(), 2)
    assert torch.equal(_levels_agree(a.cuda(), b.cuda(), 2).cpu(), expected)


@pytest.mark.parametrize('bpp', [1, 3])
def test_one_window_past_a_tile_edge_each_way(hip_lib, bpp):
    M = _m()
    h, w = M.TILE_H + 11, M.TILE_W + 11                                           # 27 x 43: 17 x 33 windows, the next level 13 x 21
    a = clip(2, h, w, bpp, seed=130 + bpp)
    b = disturbed(a, seed=131 + bpp)
    expected = _agrees(a.cuda(), b.cuda(), 2)
    assert expected[0, 0, :, 2].tolist() == [(M.TILE_H + 1) * (M.TILE_W + 1), (h // 2 - 10) * (w // 2 - 10)]
    assert torch.equal(_levels_agree(a.cuda(), b.cuda(), 2).cpu(), expected)


@pytest.mark.parametrize('bpp', [1, 2, 3, 4])
def test_canvas_views_and_strided_frames_are_read_in_place(hip_lib, bpp):
    M = _m()
    a = clip(2, 45, 47, bpp, seed=140 + bpp)
    b = disturbed(a, seed=150 + bpp)
    expected = M.msssim_sums(a, b, 3)
    va, vb = in_canvas(a.cuda()), in_canvas(b.cuda(), pad=(4, 6), frame_step=3)
    assert not va.is_contiguous() and va.stride(1) % 4 == (3, 2, 1, 0)[bpp - 1] and va.stride() != vb.stride()
    for fused in (True, False):
        assert torch.equal(M.msssim_sums(va, vb, 3, fused=fused).cpu(), expected), fused
    for pad in ((0, 0), (1, 1), (2, 3), (5, 2)):                                  # every alignment of a row's first byte
        view = in_canvas(a.cuda(), pad=pad, frame_step=1)
        assert torch.equal(M.halve(view).cpu(), M.halve(a)), pad
        assert torch.equal(M.msssim_sums(view, vb, 2).cpu(), expected[:, :, :2]), pad
    canvas = torch.full([3, 30, 31] + list(a.shape[3:]), 0xA5, dtype=torch.uint8, device='cuda')
    for x in (1, 2, 3, 4):                                                        # and of an output row's
        out = canvas[1:, 3:25, x:x + 23]
        assert M.halve(va, out=out) is out and torch.equal(out.cpu(), M.halve(a)), x
        out.fill_(0xA5)
        assert bool((canvas == 0xA5).all()), 'a store left the window'


@pytest.mark.parametrize('bpp', [1, 2, 3, 4])
def test_halve_at_sizes_around_a_lane_and_a_tile(hip_lib, bpp):
    """A lane owns 4 output bytes (12 at three bytes a pixel) and a work-group 64 lanes by 16 rows: rows that end inside a lane's bytes, one lane, one
    work-group and a pixel either way, and sides of 1, 2 and 3."""
    M = _m()
    group = 12 if bpp == 3 else 4
    lane_pixels, tile_pixels = group // bpp, 64 * group // bpp
    widths = sorted({2, 3, 4, 5, 2 * lane_pixels + 2, 4 * lane_pixels + 2, 2 * tile_pixels - 2, 2 * tile_pixels, 2 * tile_pixels + 3})
    for n, w in enumerate(widths):
        for h in (2, 3, 31, 32, 35):
            a = clip(2, h, w, bpp, seed=160 + n)
            assert torch.equal(M.halve(a.cuda()).cpu(), M.halve(a)), (h, w, bpp)
    for h, w in ((1, 1), (1, 9), (9, 1)):
        a = clip(2, h, w, bpp, seed=170)
        n, out = _launches(lambda: M.halve(a.cuda()))
        assert n == 0 and out.is_cuda and tuple(out.shape) == (2, h // 2, w // 2) + tuple(a.shape[3:])
    assert _launches(lambda: M.halve(clip(2, 6, 8, bpp, seed=171).cuda()))[0] == 1


@pytest.mark.parametrize('bpp', [1, 2, 3, 4])
def test_one_level_is_ssim_sums_on_the_device(hip_lib, bpp):
    """The two kernels share one window core: their sums are the same bytes, and the CPU formulation's."""
    from pix2pix3d_amd import quality
    for n, (f, h, w) in enumerate(SINGLE_LEVEL_SIZES):
        a = clip(f, h, w, bpp, seed=24 + n)
        b = disturbed(a, seed=26 + n)
        assert torch.equal(single_level_agrees(a.cuda(), b.cuda()).cpu(), quality.ssim_sums(a, b))


def test_extremes_on_the_device(hip_lib):
    M = _m()
    board, inverse = checkerboard(1, 44, 44, 2)
    flat = torch.full([1, 44, 44, 2], 40, dtype=torch.uint8)
    for a, b in ((board, inverse), (board, board), (flat, 255 - flat), (board, flat)):
        _agrees(a.cuda(), b.cuda(), 3)
    opposed = M.msssim_sums(board.cuda(), inverse.cuda(), 3)
    assert bool((opposed[:, :, 0, 1] < 0).all()) and M.metrics_from_msssim(opposed)['ms_ssim'] == 0.0


def test_two_calls_accumulate_without_a_synchronisation(hip_lib):
    M = _m()
    a = clip(2, 44, 50, 3, seed=180)
    b, c = disturbed(a, seed=181), disturbed(a, seed=182)
    da, db, dc = a.cuda(), b.cuda(), c.cuda()
    M.msssim_sums(da, db, 3)                                                      # (the first call loads the library and the code object)
    out = torch.zeros([2, 3, 3, 3], dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            n, _ = _launches(lambda: (M.msssim_sums(da, db, 3, out=out), M.msssim_sums(da, dc, 3, out=out)))
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    assert [str(w.message) for w in caught if 'called a synchronizing' in str(w.message)] == []
    assert n == 2 * 3 and torch.equal(out.cpu(), M.msssim_sums(a, b, 3) + M.msssim_sums(a, c, 3))
    acc = M.MultiScale('cuda', bpp=3, levels=3)
    acc.add(da, db)
    acc.add(da[:1], dc[:1])
    host = M.MultiScale('cpu', bpp=3, levels=3)
    host.add(a, b)
    host.add(a[:1], c[:1])
    assert acc.result() == host.result() and acc.result()['frames'] == 3


def test_no_frame_launches_nothing(hip_lib):
    M = _m()
    a = clip(2, 44, 50, 3, seed=190).cuda()
    for fused in (True, False):
        n, sums = _launches(lambda: M.msssim_sums(a[:0], a[:0], 3, fused=fused))
        assert n == 0 and sums.is_cuda and tuple(sums.shape) == (0, 3, 3, 3)
    n, out = _launches(lambda: M.halve(a[:0]))
    assert n == 0 and out.is_cuda and tuple(out.shape) == (0, 22, 25, 3)
    out = torch.ones([2, 3, 3, 3], dtype=torch.int64, device='cuda')
    with pytest.raises(ValueError):
        M.msssim_sums(a, a, 4)                                                    # too small: before any launch
    with pytest.raises(ValueError):
        M.msssim_sums(a, a.cpu(), 3)
    with pytest.raises(ValueError):
        M.msssim_sums(a, a, 3, out=out.cpu())
    assert bool((out == 1).all())


def test_the_ms_ssim_target_of_the_quality_search(hip_lib):
    """On a 176 x 176 clip: the returned quality meets the target as measured on the device, the next lower one does not, and the host search agrees."""
    from pix2pix3d_amd import video
    M = _m()
    frames, _ = pairs(176, 176)['smooth']
    target = 0.97
    quality, metrics, met = video.jpeg_quality_for(frames.cuda(), ms_ssim=target)
    assert met and 1 < quality < 100 and metrics['ms_ssim'] >= target
    assert metrics == M.ms_ssim(video.jpeg_reconstruct(frames.cuda(), quality), frames.cuda())
    assert M.ms_ssim(video.jpeg_reconstruct(frames.cuda(), quality - 1), frames.cuda())['ms_ssim'] < target
    assert (quality, metrics, met) == video.jpeg_quality_for(frames, ms_ssim=target)
    assert video.jpeg_quality_for(frames.cuda(), ms_ssim=1.0)[::2] == (100, False)
