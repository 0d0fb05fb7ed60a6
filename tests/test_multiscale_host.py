"""pix2pix3d_amd.multiscale without a GPU: the torch formulation — the definition — against a plain per-window Python loop, level by level against
``quality.ssim_sums`` on the pyramid, ``halve`` against its integer rule, the fixed points, every argument error, the distance to the textbook float
formulation, one level against ``quality.ssim_sums``, where the prototypes stand, and the argument checks of the two entry points (which come before any device call)."""
import ctypes

import numpy as np
import pytest
import torch

from multiscale_cases import SINGLE_LEVEL_SIZES, halve_rule, msssim_loop, msssim_true, pairs, single_level_agrees
from quality_cases import checkerboard, clip, disturbed, in_canvas

# The largest |ms_ssim - msssim_true| measured on the CPU over ``pairs()`` at five levels and the 'smooth' pair at one to four: 5.602e-4, on 'smooth' at two
# levels (five levels: random 4.7e-5, smooth 3.63e-4, disturbed 4.2e-5, jpeg q30 4:2:0 4.905e-4, jpeg q75 4:4:4 3.0e-5; 'smooth' at 1 / 2 / 3 / 4 levels
# 3.2e-5 / 5.602e-4 / 3.90e-4 / 3.97e-4) — nearly all of it the rounding of the pyramid's samples to uint8, which the float pooling does not have.  The bound
# is 3 x that measurement, the project's convention for measured bounds.
FLOAT_DEVIATION_MEASURED = 5.602e-4
FLOAT_DEVIATION_BOUND = 3 * FLOAT_DEVIATION_MEASURED


def _m():
    from pix2pix3d_amd import multiscale
    return multiscale


def test_the_definition_equals_a_plain_loop_over_windows():
    M = _m()
    a = clip(1, 22, 23, 2, seed=3)
    b = disturbed(a, seed=4)
    sums = M.msssim_sums(a, b, levels=2)
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (1, 2, 2, 3)
    assert sums.tolist() == msssim_loop(a.numpy(), b.numpy(), 2)
    assert sums[0, :, :, 2].tolist() == [[12 * 13, 1 * 1]] * 2                      # 22 x 23 and 11 x 11: the last level is a single window
    grey = clip(2, 23, 22, 1, seed=5)
    assert M.msssim_sums(grey, disturbed(grey, seed=6), levels=2).tolist() == msssim_loop(grey.numpy(), disturbed(grey, seed=6).numpy(), 2)


@pytest.mark.parametrize('bpp', [1, 3])
def test_every_level_agrees_with_ssim_sums_on_the_pyramid(bpp):
    from pix2pix3d_amd import quality
    M = _m()
    a = clip(2, 177, 190, bpp, seed=10 + bpp)
    b = disturbed(a, seed=20 + bpp)
    sums = M.msssim_sums(a, b)
    pa, pb = M.pyramid(a), M.pyramid(b)
    assert pa[0] is a and [tuple(t.shape[1:3]) for t in pa] == [(177, 190), (88, 95), (44, 47), (22, 23), (11, 11)]
    for k in range(5):
        assert torch.equal(sums[:, :, k, [0, 2]], quality.ssim_sums(pa[k], pb[k])), k
    assert int(sums[..., 1].min()) > 0 and not torch.equal(sums[..., 0], sums[..., 1])


@pytest.mark.parametrize('bpp', [1, 2, 3, 4])
def test_one_level_is_ssim_sums(bpp):
    for n, (f, h, w) in enumerate(SINGLE_LEVEL_SIZES):
        a = clip(f, h, w, bpp, seed=24 + n)
        sums = single_level_agrees(a, disturbed(a, seed=26 + n))
        assert sums[0, :, 1].tolist() == [(h - 10) * (w - 10)] * bpp


@pytest.mark.parametrize('module', ['resample', 'multiscale', 'quality', 'decimate'])
def test_the_import_pulls_in_no_session(module):
    """The frame and mesh modules stand below the sessions: importing one leaves ``sketch``, ``views`` and ``edit`` unimported (a fresh interpreter each)."""
    import pathlib
    import subprocess
    import sys
    child = (f'import sys; import pix2pix3d_amd.{module}; '
             'found = [m for m in ("sketch", "views", "edit") if "pix2pix3d_amd." + m in sys.modules]; assert not found, found')
    r = subprocess.run([sys.executable, '-c', child], capture_output=True, text=True, cwd=pathlib.Path(__file__).resolve().parent.parent)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize('bpp', [1, 2, 3, 4])
def test_halve_is_the_integer_rule(bpp):
    M = _m()
    for n, (h, w) in enumerate(((1, 1), (1, 7), (6, 1), (2, 2), (3, 3), (5, 8), (8, 5), (13, 22), (16, 33))):
        a = clip(2, h, w, bpp, seed=30 + n)
        got = M.halve(a)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2, h // 2, w // 2) + tuple(a.shape[3:])
        assert np.array_equal(got.numpy(), halve_rule(a.numpy())), (h, w, bpp)
        view = in_canvas(a)
        assert not view.is_contiguous() and torch.equal(M.halve(view), got)
    a = clip(3, 13, 22, bpp, seed=40)
    canvas = torch.full([4, 9, 14] + list(a.shape[3:]), 0xA5, dtype=torch.uint8)
    out = canvas[1:, 2:8, 1:12]
    assert M.halve(a, out=out) is out and np.array_equal(out.numpy(), halve_rule(a.numpy()))
    out.fill_(0xA5)
    assert bool((canvas == 0xA5).all())
    levels = M.pyramid(a, 3)
    assert [tuple(t.shape[1:3]) for t in levels] == [(13, 22), (6, 11), (3, 5)] and np.array_equal(levels[2].numpy(), halve_rule(halve_rule(a.numpy())))


def test_halve_rounds_once_per_sample():
    """(sum + 2) >> 2: halves round up, and there is ONE rounding (``resize(..., 'box')`` rounds once per pass and is a different rule; nothing here
    compares the two)."""
    assert _m().halve(torch.tensor([[[0, 1], [1, 1]]], dtype=torch.uint8)).tolist() == [[[1]]]          # 5 >> 2
    assert _m().halve(torch.tensor([[[0, 1], [1, 0]]], dtype=torch.uint8)).tolist() == [[[1]]]          # 4 >> 2: 0.5 rounds up
    assert _m().halve(torch.tensor([[[0, 0], [1, 0]]], dtype=torch.uint8)).tolist() == [[[0]]]      # 3 >> 2
    assert _m().halve(torch.tensor([[[255, 255], [255, 254]]], dtype=torch.uint8)).tolist() == [[[255]]]


def test_fixed_points():
    M = _m()
    a = clip(2, 44, 47, 3, seed=50)
    same = M.msssim_sums(a, a, levels=3)
    assert torch.equal(same[..., 0], same[..., 2] << 32) and torch.equal(same[..., 1], same[..., 2] << 32)      # every contribution exactly 2^32
    assert same[0, 0, :, 2].tolist() == [34 * 37, 12 * 13, 1]
    metrics = M.metrics_from_msssim(same)
    assert metrics['ms_ssim'] == 1.0 and metrics['level_cs'] == [1.0] * 3 and metrics['level_q'] == [1.0] * 3
    assert metrics['frame_channel_ms_ssim'] == [[1.0] * 3] * 2 and metrics['channel_ms_ssim'] == [1.0] * 3 and metrics['frame_ms_ssim'] == [1.0] * 2
    assert (metrics['frames'], metrics['channels'], metrics['levels'], metrics['windows']) == (2, 3, 3, [2 * 34 * 37, 2 * 12 * 13, 2])
    assert M.ms_ssim(a, a, 3) == metrics
    flat, other = torch.full([1, 44, 44], 40, dtype=torch.uint8), torch.full([1, 44, 44], 200, dtype=torch.uint8)
    constant = M.msssim_sums(flat, other, levels=3)
    assert torch.equal(constant[..., 1], constant[..., 2] << 32)                   # no variance on either side: cs = C2 / C2 = 1 at every level
    assert bool((constant[..., 0] < constant[..., 1]).all())                       # and the luminance term says that the means differ
    board, inverse = checkerboard(1, 44, 44, 2)
    opposed = M.msssim_sums(board, inverse, levels=3)
    assert bool((opposed[:, :, 0, 1] < 0).all()) and bool((opposed[:, :, 0, 0] < 0).all())      # negative cs sums at level 0
    clamped = M.metrics_from_msssim(opposed)
    assert clamped['ms_ssim'] == 0.0 and clamped['level_cs'][0] < -0.9 and clamped['frame_channel_ms_ssim'] == [[0.0, 0.0]]


def test_out_accumulates_and_no_frame_adds_nothing():
    M = _m()
    a = clip(2, 22, 30, 2, seed=60)
    b = disturbed(a, seed=61)
    once = M.msssim_sums(a, b, levels=2)
    out = torch.zeros([2, 2, 2, 3], dtype=torch.int64)
    assert M.msssim_sums(a, b, levels=2, out=out) is out and M.msssim_sums(a, b, levels=2, out=out) is out
    assert torch.equal(out, 2 * once)
    assert torch.equal(M.msssim_sums(a, b, levels=2, fused=False), once)           # the switch plays no part on the CPU
    empty = M.msssim_sums(a[:0], b[:0], levels=2)
    assert tuple(empty.shape) == (0, 2, 2, 3) and empty.dtype == torch.int64
    assert np.isnan(M.metrics_from_msssim(empty)['ms_ssim']) and M.metrics_from_msssim(empty)['frames'] == 0
    assert tuple(M.halve(a[:0]).shape) == (0, 11, 15, 2)


def test_weights_and_the_accumulator():
    M = _m()
    assert M.WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) and abs(sum(M.default_weights(5)) - 1) < 1e-15
    assert M.default_weights(2) == (0.0448 / (0.0448 + 0.2856), 0.2856 / (0.0448 + 0.2856)) and M.default_weights(1) == (1.0,)
    assert [M.min_size(k) for k in range(1, 6)] == [11, 22, 44, 88, 176] and M.min_size() == 176
    a = clip(3, 44, 50, 3, seed=70)
    b = disturbed(a, seed=71)
    sums = M.msssim_sums(a, b, levels=3)
    default, last_only = M.metrics_from_msssim(sums), M.metrics_from_msssim(sums, weights=(0, 0, 1))
    s = sums.tolist()
    q2 = [[s[i][c][2][0] / (s[i][c][2][2] * 2.0 ** 32) for c in range(3)] for i in range(3)]
    assert last_only['frame_channel_ms_ssim'] == q2 and last_only['weights'] == [0.0, 0.0, 1.0]
    cell = s[1][2]
    cs = [cell[k][1] / (cell[k][2] * 2.0 ** 32) for k in range(3)]
    w = M.default_weights(3)
    assert default['frame_channel_ms_ssim'][1][2] == pytest.approx(cs[0] ** w[0] * cs[1] ** w[1] * q2[1][2] ** w[2], rel=1e-15)
    assert default['ms_ssim'] == pytest.approx(np.mean(default['frame_channel_ms_ssim']), rel=1e-15)
    assert default['channel_ms_ssim'][0] == pytest.approx(np.mean([default['frame_channel_ms_ssim'][i][0] for i in range(3)]), rel=1e-15)
    assert M.ms_ssim(a, b, 3, weights=(0, 0, 1)) == last_only
    acc = M.MultiScale('cpu', bpp=3, levels=3)
    acc.add(a[:2], b[:2])
    acc.add(a[2:], b[2:])
    result = acc.result()
    pooled = M.metrics_from_msssim(sums.sum(dim=0, keepdim=True))
    assert result['frames'] == 3 and {k: v for k, v in result.items() if k != 'frames'} == {k: v for k, v in pooled.items() if k != 'frames'}
    assert result['level_cs'] == default['level_cs'] and result['level_q'] == default['level_q']


def test_python_refuses_bad_arguments():
    from pix2pix3d_amd import video
    M = _m()
    a = clip(2, 44, 45, 3, seed=80)
    bad = [lambda: M.msssim_sums(a, a[:, :, :44]), lambda: M.msssim_sums(a, a[:1]), lambda: M.msssim_sums(a, a[..., 0]),      # shapes
           lambda: M.msssim_sums(a.float(), a.float()), lambda: M.msssim_sums(a, a.numpy()), lambda: M.msssim_sums(a, a.to('meta')),      # dtype, device
           lambda: M.msssim_sums(a[:, :, ::2], a[:, :, ::2], levels=1),                                                       # pixels apart
           lambda: M.msssim_sums(a, a, levels=0), lambda: M.msssim_sums(a, a, levels=6), lambda: M.msssim_sums(a, a, levels=2.0),
           lambda: M.msssim_sums(a, a, levels=True), lambda: M.pyramid(a, 6), lambda: M.min_size(0), lambda: M.default_weights(7),
           lambda: M.msssim_sums(a, a, levels=4),                                                                            # too small
           lambda: M.msssim_sums(a, a, levels=3, out=torch.zeros([2, 3, 3, 3], dtype=torch.int32)),
           lambda: M.msssim_sums(a, a, levels=3, out=torch.zeros([2, 3, 2, 3], dtype=torch.int64)),
           lambda: M.msssim_sums(a, a, levels=3, out=torch.zeros([2, 3, 3, 6], dtype=torch.int64)[..., ::2]),
           lambda: M.ms_ssim(a, a, 3, weights=(0.5, 0.5)), lambda: M.ms_ssim(a, a, 3, weights=(0.5, -0.1, 0.6)), lambda: M.ms_ssim(a, a, 3, weights='abc'),
           lambda: M.metrics_from_msssim(torch.zeros([2, 3, 3, 3], dtype=torch.int64), weights=(1, 1)),
           lambda: M.metrics_from_msssim(torch.zeros([2, 3, 3], dtype=torch.int64)), lambda: M.metrics_from_msssim(torch.zeros([2, 3, 3, 3])),
           lambda: M.halve(a.float()), lambda: M.halve(a, out=torch.zeros([2, 22, 22, 4], dtype=torch.uint8)), lambda: M.halve(a, out=a[:, :22, :22]),
           lambda: M.MultiScale('cpu', bpp=5), lambda: M.MultiScale('cpu', levels=0), lambda: M.MultiScale('cpu', bpp=1).add(a, a),
           lambda: M.level_sums(a, a, torch.zeros([2, 3, 3, 3], dtype=torch.int64), 0),                                       # the entry point is the device's
           lambda: video.jpeg_quality_for(a, ssim=0.9, ms_ssim=0.9), lambda: video.jpeg_quality_for(a, psnr=30.0, ms_ssim=0.9),
           lambda: video.jpeg_quality_for(a, psnr=30.0, ssim=0.9, ms_ssim=0.9), lambda: video.jpeg_quality_for(a, ms_ssim=1.5),
           lambda: video.jpeg_quality_for(a, ms_ssim=0.9),                                                                   # 44 x 45: too small for five levels
           lambda: video.encode_jpeg(a, ssim=0.9, ms_ssim=0.9), lambda: video.save_avi('never_written.avi', a, psnr=30.0, ms_ssim=0.9)]
    for n, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f'case {n} raised nothing')
    with pytest.raises(ValueError, match=r'admits levels <= 3'):
        M.msssim_sums(a, a, levels=4)
    with pytest.raises(ValueError, match=r'admits levels <= 4'):
        M.msssim_sums(clip(1, 175, 300, 1, seed=81), clip(1, 175, 300, 1, seed=81))
    with pytest.raises(ValueError, match=r'no level at all'):
        M.msssim_sums(a[:, :10], a[:, :10], levels=1)
    wide = clip(1, 176, 176, 1, seed=82)
    assert M.msssim_sums(wide, wide)[0, 0, 4].tolist() == [1 << 32, 1 << 32, 1]       # 176 passes: one window at the fifth level


def test_the_float_formulation_is_close():
    """|ms_ssim - textbook| on the random, smooth, disturbed and JPEG-degraded clips at five levels, and on the smooth pair at fewer: each is printed, the
    largest stays under 3 x the measured 5.602e-4."""
    M = _m()
    worst = 0.0
    for name, levels in [(name, 5) for name in pairs()] + [('smooth', levels) for levels in (1, 2, 3, 4)]:
        a, b = pairs()[name]
        got, true = M.ms_ssim(a, b, levels)['ms_ssim'], msssim_true(a.numpy(), b.numpy(), levels)
        print(f'{name}, {levels} levels: ms_ssim {got:.9f}, float formulation {true:.9f}, |difference| {abs(got - true):.3e}')
        worst = max(worst, abs(got - true))
    print(f'largest |difference| {worst:.4e}; measured {FLOAT_DEVIATION_MEASURED:.4e}, bound {FLOAT_DEVIATION_BOUND:.4e}')
    assert worst <= FLOAT_DEVIATION_BOUND


def test_the_target_reaches_the_writers(tmp_path):
    """``ms_ssim=`` wherever ``psnr=`` and ``ssim=`` go, with the post-condition of the search; the existing calls write the bytes they wrote."""
    from pix2pix3d_amd import video
    M = _m()
    a, _ = pairs(176, 176)['smooth']
    quality, metrics, met = video.jpeg_quality_for(a, ms_ssim=0.97)
    assert met and 1 < quality < 100 and metrics == M.ms_ssim(video.jpeg_reconstruct(a, quality), a) and metrics['ms_ssim'] >= 0.97
    assert M.ms_ssim(video.jpeg_reconstruct(a, quality - 1), a)['ms_ssim'] < 0.97
    assert video.jpeg_quality_for(a, ms_ssim=1.0)[::2] == (100, False)
    streams = video.save_avi(tmp_path / 'a.avi', a, ms_ssim=0.97)
    assert streams == video.encode_jpeg(a, quality) == video.encode_jpeg(a, ms_ssim=0.97) == video.read_avi(tmp_path / 'a.avi')[0]
    assert video.save_clip(tmp_path / 'b.avi', a, format='avi', ms_ssim=0.97) == (quality, metrics, met)
    assert (tmp_path / 'b.avi').read_bytes() == (tmp_path / 'a.avi').read_bytes()
    with pytest.raises(ValueError):
        video.save_clip(tmp_path / 'c.gif', a, format='gif', ms_ssim=0.97)
    assert video.jpeg_quality_for(a, ssim=0.9) == video.jpeg_quality_for(a, None, 0.9, '4:2:0', 8)      # the positional order stands


def test_where_the_prototypes_stand():
    from pix2pix3d_amd import _lib, clips, decimate, regions, sketch
    M = _m()
    new = ['p3d_frame_halve', 'p3d_frame_msssim_level']                             # declared by the video header and by no other
    assert all(n in clips.HEADER.functions for n in new)
    assert not any(n in header.functions for n in new for header in (_lib.HEADER, regions.HEADER, sketch.HEADER, decimate.HEADER))
    assert [len(clips.HEADER.functions[n][1]) for n in new] == [11, 15]
    constants = clips.HEADER.constants
    assert (M.TILE_W, M.TILE_H, M.MAX_LEVELS) == (constants['P3D_MSSSIM_TILE_W'], constants['P3D_MSSSIM_TILE_H'], constants['P3D_MSSSIM_MAX_LEVELS']) == (32, 16, 5)
    assert M.TILE_W % 2 == 0 and M.TILE_H % 2 == 0


def test_the_library_refuses_bad_arguments_before_any_launch():
    from pix2pix3d_amd import _lib, clips
    lib, n0 = clips.video_lib(), clips.launch_count()
    buffer = ctypes.create_string_buffer(4096)                                     # host memory: no call below may get as far as reading it
    p = ctypes.cast(buffer, ctypes.c_void_p)
    level = lambda a, b, f, h, w, bpp, sums=p, pitch=3, na=None, nb=None, row=48: lib.p3d_frame_msssim_level(a, 1024, row, b, 1024, 48, f, h, w, bpp, sums, pitch,
                                                                                                            na, nb, None)
    assert level(p, p, 1, 12, 12, 0) == _lib.P3D_ERR_ARGUMENT and b'bpp' in lib.p3d_last_error()
    assert level(p, p, 1, 12, 12, 5) == _lib.P3D_ERR_ARGUMENT and level(p, p, -1, 12, 12, 3) == _lib.P3D_ERR_ARGUMENT
    assert level(p, p, 1, -12, 12, 3) == _lib.P3D_ERR_ARGUMENT and level(p, p, 1, 12, -12, 3) == _lib.P3D_ERR_ARGUMENT
    assert level(None, p, 1, 12, 12, 3) == _lib.P3D_ERR_ARGUMENT and level(p, None, 1, 12, 12, 3) == _lib.P3D_ERR_ARGUMENT
    assert level(p, p, 1, 12, 12, 3, sums=None) == _lib.P3D_ERR_ARGUMENT
    assert level(p, p, 1, 12, 12, 3, pitch=2) == _lib.P3D_ERR_ARGUMENT
    assert level(p, p, 1, 10, 12, 3) == _lib.P3D_ERR_ARGUMENT and b'window' in lib.p3d_last_error()      # a level without a window is an error
    assert level(p, p, 1, 12, 10, 3) == _lib.P3D_ERR_ARGUMENT
    assert level(p, p, 1, 12, 12, 3, row=35) == _lib.P3D_ERR_ARGUMENT               # a row pitch under w bpp
    assert level(p, p, 1, 12, 12, 3, na=p) == _lib.P3D_ERR_ARGUMENT and level(p, p, 1, 12, 12, 3, nb=p) == _lib.P3D_ERR_ARGUMENT
    assert level(p, p, 1, 12, 12, 3, na=p, nb=p) == _lib.P3D_ERR_ARGUMENT           # one buffer for both
    assert level(p, p, 2, 1 << 15, 1 << 15, 1) == _lib.P3D_ERR_ARGUMENT             # 2^31 samples
    assert level(None, None, 0, 12, 12, 3, sums=None) == _lib.P3D_OK                # no frame: nothing to read, nothing to do
    assert level(None, None, 3, 0, 12, 3, sums=None) == _lib.P3D_OK
    halve = lambda src, dst, f, h, w, bpp, srow=48, drow=24, dframe=1024: lib.p3d_frame_halve(src, 1024, srow, f, h, w, bpp, dst, dframe, drow, None)
    q = ctypes.cast(ctypes.addressof(buffer) + 2048, ctypes.c_void_p)
    assert halve(p, q, 1, 12, 12, 0) == _lib.P3D_ERR_ARGUMENT and halve(p, q, 1, 12, 12, 5) == _lib.P3D_ERR_ARGUMENT
    assert halve(p, q, -1, 12, 12, 3) == _lib.P3D_ERR_ARGUMENT and halve(p, q, 1, -1, 12, 3) == _lib.P3D_ERR_ARGUMENT
    assert halve(None, q, 1, 12, 12, 3) == _lib.P3D_ERR_ARGUMENT and halve(p, None, 1, 12, 12, 3) == _lib.P3D_ERR_ARGUMENT
    assert halve(p, q, 1, 12, 12, 3, srow=35) == _lib.P3D_ERR_ARGUMENT and halve(p, q, 1, 12, 12, 3, drow=17) == _lib.P3D_ERR_ARGUMENT
    assert halve(p, q, 2, 12, 12, 3, dframe=100) == _lib.P3D_ERR_ARGUMENT           # the destination's frames overlap
    assert halve(p, p, 1, 12, 12, 3) == _lib.P3D_ERR_ARGUMENT and b'out of place' in lib.p3d_last_error()
    assert halve(None, None, 0, 12, 12, 3) == _lib.P3D_OK and halve(None, None, 2, 1, 12, 3) == _lib.P3D_OK and halve(None, None, 2, 12, 1, 3) == _lib.P3D_OK
    assert clips.launch_count() == n0
