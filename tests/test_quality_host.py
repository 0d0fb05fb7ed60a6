"""Frame quality on the host (pix2pix3d_amd/quality.py, the decode side of video/jpeg.py): the torch formulations — the definitions the
device kernels must equal — against first principles, the fixed-point SSIM window against the true Gaussian, the decoder against an fp64 inverse and
against PIL, the post-condition of the quality search, and the argument checks of the library and of Python.  No GPU: the library's checks run before any
device call."""
import ctypes
import math
import pathlib
import re

import numpy as np
import pytest
import torch

from conftest import record_error
from jpeg_cases import PICTURES, SUBSAMPLINGS, decode, frames_of, psnr
from quality_cases import (C1, C2, DECODE_MARGIN_DB, WINDOW, checkerboard, clip, disturbed, grey, idct_fp64, in_canvas, ssim_loop, ssim_true)
from video_cases import gradient_frames, noise_frames

# 3 x the worst value measured on the CPU (the project's convention for parity bounds; the measurements are in DESIGN.md section 2.1x)
SSIM_WINDOW_BOUND = 3 * 9.38e-5                      # |mean SSIM by the integer rules - by the true Gaussian in fp64|: worst 9.38e-5 ('gradient' at quality 30)
DECODE_LEVEL_BOUND = 3 * 0.5642                      # |decoded sample - the fp64 inverse before rounding|, grey levels: worst 0.5642 (grey 'noise' at quality 90)


def _q():
    from pix2pix3d_amd import quality
    return quality


def _video():
    from pix2pix3d_amd import video
    return video


# ---- the rules ---------------------------------------------------------------------------------------------------------------------------------
def test_the_window_and_the_constants_equal_their_formulas_and_the_header():
    Q, video = _q(), _video()
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5)
    assert tuple(np.round(1024 * g / g.sum()).astype(int)) == WINDOW == tuple(Q.ssim_window().tolist()) and sum(WINDOW) == 1024
    from pix2pix3d_amd import build
    text = pathlib.Path(build.side_paths('video').header).read_text()
    literal = re.search(r'#define P3D_VIDEO_SSIM_WINDOW ([\d, ]+)', text).group(1)
    assert tuple(int(v) for v in literal.split(',')) == WINDOW
    assert (Q.C1, Q.C2) == (C1, C2) == (round((0.01 * 255) ** 2 * 2 ** 40), round((0.03 * 255) ** 2 * 2 ** 40))
    assert (Q.TAPS, Q.SHIFT) == (11, 32)


def test_ssim_equals_a_plain_loop_over_windows():
    Q = _q()
    a = clip(1, 13, 12, 3, seed=1)
    b = disturbed(a, seed=2)
    assert Q.ssim_sums(a, b).tolist() == ssim_loop(a, b)
    grey_a, grey_b = a[..., 1].contiguous(), b[..., 1].contiguous()
    assert Q.ssim_sums(grey_a, grey_b).tolist() == [[ssim_loop(a, b)[0][1]]]        # [F, H, W] is bpp = 1


def test_identical_frames_give_exactly_one():
    Q = _q()
    a = clip(2, 14, 17, 3, seed=3)
    sums, maps = Q.ssim_sums(a, a, maps=True)
    assert sums.tolist() == [[[4 * 7 << 32, 4 * 7]] * 3] * 2
    assert maps.dtype == torch.float32 and tuple(maps.shape) == (2, 4, 7, 3) and bool((maps == 1).all())
    m = Q.compare(a, a)
    assert m['ssim'] == 1.0 and m['psnr'] == math.inf and m['mse'] == 0 and m['max'] == 0 and m['changed'] == 0 and m['windows'] == 56


def test_the_extreme_pair_is_negative_and_nothing_overflows():
    """x against 255 - x on a board of 0 and 255: equal means, the most negative covariance.  And the bounds the header states, on the factors themselves:
    below 2^59, d1 and d2 positive — here, on flat white (the largest A, B and d1) and on white against black."""
    Q = _q()
    a, b = checkerboard(1, 13, 12, 3)
    sums = Q.ssim_sums(a, b)
    assert sums.tolist() == ssim_loop(a, b) and int(sums[0, 0, 0]) < -(6 << 31) and sums[0, :, 1].tolist() == [6] * 3
    assert Q.compare(a, b)['ssim'] < -0.99
    white, black = torch.full([1, 11, 11], 255, dtype=torch.uint8), torch.zeros([1, 11, 11], dtype=torch.uint8)
    coarse = checkerboard(1, 21, 21, 1, cell=5)
    for x, y in ((a, b), (white, white), (white, black), coarse):
        moments = Q.ssim_moments(x, y)
        assert all(int(m.min()) >= 0 for m in moments) and max(int(m.max()) for m in moments[:2]) < 2 ** 28 and max(int(m.max()) for m in moments[2:]) < 2 ** 36
        n1, n2, d1, d2 = Q.ssim_factors(moments)
        assert max(int(t.abs().max()) for t in (n1, n2, d1, d2)) < 2 ** 59 and int(d1.min()) >= C1 and int(d2.min()) >= C2
    assert Q.ssim_sums(white, white).tolist() == [[[1 << 32, 1]]]


def test_too_small_for_a_window():
    Q = _q()
    a = clip(2, 10, 40, 3, seed=4)
    b = disturbed(a, seed=5)
    sums, maps = Q.ssim_sums(a, b, maps=True)
    assert sums.tolist() == [[[0, 0]] * 3] * 2 and tuple(maps.shape) == (2, 0, 30, 3)
    m = Q.compare(a, b)
    assert math.isnan(m['ssim']) and all(math.isnan(v) for v in m['channel_ssim'] + m['frame_ssim']) and m['windows'] == 0 and m['psnr'] > 0
    empty = Q.compare(a[:0], b[:0])
    assert math.isnan(empty['psnr']) and math.isnan(empty['mae']) and math.isnan(empty['ssim']) and empty['frames'] == 0 and empty['max'] == 0


@pytest.mark.parametrize('bpp', [1, 2, 3, 4])
def test_error_sums_equal_numpy_on_pitched_views(bpp):
    Q = _q()
    a = clip(3, 9, 14, bpp, seed=6)
    b = disturbed(a, seed=7)
    d = np.abs(a.numpy().astype(np.int64) - b.numpy().astype(np.int64)).reshape(3, 9 * 14, bpp)
    expected = np.stack([d.sum(axis=1), (d * d).sum(axis=1), d.max(axis=1), (d != 0).sum(axis=1)], axis=2)
    va, vb = in_canvas(a), in_canvas(b, pad=(3, 5), frame_step=3)
    assert not va.is_contiguous() and va.stride() != vb.stride()
    out = Q.error_sums(va, vb)
    assert out.dtype == torch.int64 and out.numpy().tolist() == expected.tolist()
    assert Q.error_sums(va, vb, out=out) is out                                     # a second call accumulates: sums double, the maximum stays
    expected[..., [0, 1, 3]] *= 2
    assert out.numpy().tolist() == expected.tolist()
    assert Q.ssim_sums(va, vb).tolist() == Q.ssim_sums(a, b).tolist()               # (9 rows: no window) ...
    wide_a, wide_b = clip(2, 12, 15, bpp, seed=8), clip(2, 12, 15, bpp, seed=9)
    assert Q.ssim_sums(in_canvas(wide_a), in_canvas(wide_b)).tolist() == Q.ssim_sums(wide_a, wide_b).tolist() == ssim_loop(wide_a, wide_b)


def test_the_metrics_are_the_divisions_of_the_sums():
    Q = _q()
    a = clip(2, 12, 13, 3, seed=10)
    b = disturbed(a, seed=11)
    m = Q.compare(a, b)
    d = a.numpy().astype(np.float64) - b.numpy().astype(np.float64)
    assert m['mse'] == pytest.approx((d ** 2).mean(), rel=1e-12) and m['mae'] == pytest.approx(np.abs(d).mean(), rel=1e-12) and m['max'] == np.abs(d).max()
    assert m['psnr'] == pytest.approx(psnr(a.numpy(), b.numpy()), rel=1e-12) and m['changed'] == pytest.approx((d != 0).mean(), rel=1e-12)
    assert m['frame_psnr'] == pytest.approx([psnr(a[i].numpy(), b[i].numpy()) for i in range(2)], rel=1e-12)
    assert m['channel_mse'] == pytest.approx([(d[..., c] ** 2).mean() for c in range(3)], rel=1e-12)
    s = Q.ssim_sums(a, b).numpy().astype(np.float64)
    assert m['channel_ssim'] == pytest.approx(list(s[:, :, 0].sum(axis=0) / (s[:, :, 1].sum(axis=0) * 2.0 ** 32)), rel=1e-12)
    assert m['ssim'] == pytest.approx(np.mean(m['channel_ssim']), rel=1e-12) and (m['frames'], m['channels'], m['samples'], m['windows']) == (2, 3, 2 * 3 * 156, 12)
    assert Q.metrics_from_sums(Q.error_sums(a, b), samples=156)['psnr'] == m['psnr']
    with pytest.raises(ValueError):
        Q.metrics_from_sums(Q.error_sums(a, b))                                     # the sums do not count the samples: the caller says


def test_the_accumulator_and_the_heat_frames():
    Q = _q()
    a, b = clip(2, 12, 13, 3, seed=12), clip(3, 15, 11, 3, seed=13)
    da, db = disturbed(a, seed=14), disturbed(b, seed=15)
    total = Q.Quality('cpu')
    total.add(a, da)
    total.add(b, db)
    r, ma, mb = total.result(), Q.compare(a, da), Q.compare(b, db)
    assert r['frames'] == 5 and r['max'] == max(ma['max'], mb['max'])
    assert r['mse'] == pytest.approx((ma['mse'] * ma['samples'] + mb['mse'] * mb['samples']) / (ma['samples'] + mb['samples']), rel=1e-12)
    assert r['windows'] == ma['windows'] + mb['windows']
    with pytest.raises(ValueError):
        total.add(a[..., 0], da[..., 0])                                            # one byte a pixel into counters of three
    heat = Q.difference_map(a, da)
    m = (a.to(torch.int64) - da.to(torch.int64)).abs().amax(dim=3)
    assert heat.dtype == torch.uint8 and tuple(heat.shape) == (2, 12, 13, 3) and torch.equal(heat[..., 0].long(), (3 * m).clamp(max=255))
    assert torch.equal(heat[..., 2].long(), (3 * m - 510).clamp(0, 255)) and int(Q.difference_map(a, a).max()) == 0


# ---- the fixed-point window against the true one ----------------------------------------------------------------------------------------------
def test_the_integer_ssim_stays_with_the_true_gaussian():
    Q, video = _q(), _video()
    worst = 0.0
    for name in PICTURES:
        frames = frames_of(name)
        for quality in (30, 90):
            shown = video.jpeg_reconstruct(frames, quality)
            ours, true = Q.compare(shown, frames)['ssim'], ssim_true(shown.numpy(), frames.numpy())
            if frames.shape[1] < 11 or frames.shape[2] < 11:
                assert math.isnan(ours) and math.isnan(true)
                continue
            print(f'ssim {name} q{quality}: integer {ours:.9f} true {true:.9f} difference {abs(ours - true):.3e}')
            worst = max(worst, abs(ours - true))
    record_error('quality.ssim.window', worst)
    assert 0 < worst <= SSIM_WINDOW_BOUND


# ---- the decoder --------------------------------------------------------------------------------------------------------------------------------
def test_the_decoder_stays_with_the_fp64_inverse():
    """4:4:4 on grey pictures (R = G = B: Y is the grey level exactly and both chroma planes are 128, so no colour step intervenes): every decoded sample
    against the orthonormal fp64 inverse of the same dequantised coefficients, clamped but not rounded."""
    video = _video()
    worst = 0.0
    for name in ('checkerboard', 'gradient', 'noise'):
        picture = grey(PICTURES[name])
        h, w = picture.shape[:2]
        for quality in (50, 90):
            tables = video.jpeg_tables(quality)
            coefficients = video.jpeg_coefficients(torch.from_numpy(picture)[None], tables, '4:4:4')
            assert not coefficients[:, :, 1:].any()
            luma = video.jpeg_dequantize(coefficients, tables, '4:4:4').numpy()[0, :, 0]
            my, mx = -(-h // 8), -(-w // 8)
            reference = idct_fp64(luma).reshape(my, mx, 8, 8).transpose(0, 2, 1, 3).reshape(my * 8, mx * 8)[:h, :w].clip(0, 255)
            shown = video.jpeg_decode(coefficients, tables, h, w, '4:4:4')[0].numpy().astype(np.float64)
            worst = max(worst, float(np.abs(shown - reference[:, :, None]).max()))
    print(f'decoder against the fp64 inverse: {worst:.4f} grey levels')
    record_error('quality.decode.fp64', worst)
    assert 0 < worst <= DECODE_LEVEL_BOUND


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
@pytest.mark.parametrize('name', list(PICTURES))
def test_the_decoder_holds_pils_psnr(name, subsampling):
    video = _video()
    frames = frames_of(name)
    for quality in (50, 90):
        stream, = video.encode_jpeg(frames, quality, subsampling)
        ours, pils = psnr(video.jpeg_reconstruct(frames, quality, subsampling)[0].numpy(), PICTURES[name]), psnr(decode(stream), PICTURES[name])
        print(f'decode {name} {subsampling} q{quality}: ours {ours:.4f} dB, PIL {pils:.4f} dB')
        assert ours >= pils - DECODE_MARGIN_DB


def test_the_clamps_of_the_decoder_and_a_pitched_output():
    video = _video()
    rng = np.random.default_rng(16)
    extreme = torch.from_numpy((rng.integers(0, 2, size=[2, 9, 6, 64]) * 2046 - 1023).astype(np.int16))      # +-1023 times 255: far past int16
    tables = (torch.full([64], 255, dtype=torch.uint8),) * 2
    shown = video.jpeg_decode(extreme, tables, 37, 41, '4:2:0')
    assert tuple(shown.shape) == (2, 37, 41, 3) and int(shown.min()) == 0 and int(shown.max()) == 255
    canvas = torch.full([4, 50, 60, 3], 9, dtype=torch.uint8)
    view = canvas[::2, 5:42, 7:48]
    assert video.jpeg_decode(extreme, tables, 37, 41, '4:2:0', out=view) is view and torch.equal(view, shown)
    canvas[::2, 5:42, 7:48] = 9
    assert bool((canvas == 9).all())                                                # nothing around the window was written
    zero = (torch.zeros([64], dtype=torch.uint8),) * 2                              # a 0 entry counts as 1
    one = (torch.ones([64], dtype=torch.uint8),) * 2
    assert torch.equal(video.jpeg_decode(extreme, zero, 37, 41), video.jpeg_decode(extreme, one, 37, 41))
    assert tuple(video.jpeg_decode(extreme[:0], tables, 37, 41).shape) == (0, 37, 41, 3)


# ---- the quality search ----------------------------------------------------------------------------------------------------------------------------
def _meets(frames, quality, key, target, subsampling='4:2:0'):
    return _q().compare(_video().jpeg_reconstruct(frames, quality, subsampling), frames)[key] >= target


@pytest.mark.parametrize('case, key, target', [('gradient', 'psnr', 30.0), ('gradient', 'ssim', 0.85), ('noise', 'psnr', 12.0), ('noise', 'ssim', 0.5),
                                               ('gradient', 'psnr', 1.0)])
def test_the_quality_search_keeps_its_promise(case, key, target):
    """The post-condition, re-measured: the returned quality meets the target, the one below it does not."""
    video = _video()
    frames = gradient_frames(3, 37, 53, seed=17) if case == 'gradient' else noise_frames(3, 24, 40, seed=18)
    quality, metrics, met = video.jpeg_quality_for(frames, **{key: target})
    assert met and 1 <= quality <= 100 and metrics == _q().compare(video.jpeg_reconstruct(frames, quality), frames) and metrics[key] >= target
    assert _meets(frames, quality, key, target) and (quality == 1 or not _meets(frames, quality - 1, key, target))
    assert (quality == 1) == (target == 1.0)


def test_an_unreachable_target_says_so_and_the_sample_is_taken():
    video, Q = _video(), _q()
    frames = noise_frames(12, 24, 40, seed=19)
    quality, metrics, met = video.jpeg_quality_for(frames, psnr=80.0, sample=3)
    picked = frames[[0, 5, 11]]
    assert (quality, met) == (100, False) and metrics == Q.compare(video.jpeg_reconstruct(picked, 100), picked) and metrics['frames'] == 3
    tiny = noise_frames(1, 8, 8, seed=20)
    assert video.jpeg_quality_for(tiny, ssim=0.1)[::2] == (100, False)              # no window: NaN meets nothing
    streams = video.encode_jpeg(frames[:2], psnr=12.0)
    chosen = video.jpeg_quality_for(frames[:2], psnr=12.0)[0]
    assert streams == video.encode_jpeg(frames[:2], chosen) and 1 < chosen < 100 and video.encode_jpeg(frames[:0], psnr=12.0) == []


def test_save_avi_takes_a_target(tmp_path):
    video = _video()
    frames = gradient_frames(4, 37, 53, seed=21)
    streams = video.save_avi(tmp_path / 'a.avi', frames, ssim=0.9, subsampling='4:4:4')
    quality, _, met = video.jpeg_quality_for(frames, ssim=0.9, subsampling='4:4:4')
    assert met and video.read_avi(tmp_path / 'a.avi')[0] == streams == video.encode_jpeg(frames, quality, '4:4:4')
    assert video.save_avi(tmp_path / 'b.avi', frames) == video.encode_jpeg(frames, 90)      # the default is what it was


def test_the_gif_knobs_are_measured():
    video, Q = _video(), _q()
    frames = gradient_frames(2, 24, 31, seed=22)
    few, many = video.palettize(frames, colors=8), video.palettize(frames, colors=256, palette='frame')
    a, b = video.palette_quality(frames, few[0], few[1]), video.palette_quality(frames, many[0], many[1])
    assert a == Q.compare(few[1][few[0].long()], frames) and b['psnr'] > a['psnr'] + 3 and b['frames'] == 2


def test_generate_video_takes_the_target(tmp_path):
    from model_cases import build_generator
    from pix2pix3d_amd import surface, views
    video = _video()
    G = build_generator('seg2cat', 'cpu', cbase=2048, cmax=32, depth=(6, 6), sr_num_fp16_res=0)
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(8))
    kw = dict(n_frames=2, views_per_step=2, neural_rendering_resolution=16)
    out = views.generate_video(G, ws, 'seg2cat', str(tmp_path / 'v.avi'), format='avi', ssim=0.9, **kw)
    quality, metrics, met = out['jpeg_quality']
    assert (quality, metrics, met) == video.jpeg_quality_for(out['image'], ssim=0.9)
    assert video.read_avi(tmp_path / 'v.avi')[0] == video.encode_jpeg(out['image'], quality)
    for fn in (lambda: views.generate_video(G, ws, 'seg2cat', format='gif', ssim=0.9, **kw), lambda: surface.geometry_video(G, ws, n_frames=1, psnr=30.0)):
        with pytest.raises(ValueError):
            fn()


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------------------
def test_the_library_refuses_bad_arguments_before_any_launch():
    from pix2pix3d_amd import _lib
    video = _video()
    lib, n0 = video.video_lib(), video.launch_count()
    buffer = ctypes.create_string_buffer(4096)                                     # host memory: no call below may get as far as reading it
    p = ctypes.cast(buffer, ctypes.c_void_p)
    for fn, tail in ((lib.p3d_video_error_sums, (p, None)), (lib.p3d_video_ssim, (p, None, None))):
        call = lambda a, b, f, h, w, bpp, tail=tail, row=48: fn(a, 1024, row, b, 1024, 48, f, h, w, bpp, *tail)
        assert call(p, p, 1, 12, 12, 0) == _lib.P3D_ERR_ARGUMENT and b'bpp' in lib.p3d_last_error()
        assert call(p, p, 1, 12, 12, 5) == _lib.P3D_ERR_ARGUMENT
        assert call(p, p, -1, 12, 12, 3) == _lib.P3D_ERR_ARGUMENT and call(p, p, 1, -12, 12, 3) == _lib.P3D_ERR_ARGUMENT
        assert call(p, p, 1, 12, -12, 3) == _lib.P3D_ERR_ARGUMENT
        assert call(None, p, 1, 12, 12, 3) == _lib.P3D_ERR_ARGUMENT and call(p, None, 1, 12, 12, 3) == _lib.P3D_ERR_ARGUMENT
        assert fn(p, 1024, 48, p, 1024, 48, 1, 12, 12, 3, None, *tail[1:]) == _lib.P3D_ERR_ARGUMENT      # no counters
        assert call(p, p, 1, 12, 12, 3, row=35) == _lib.P3D_ERR_ARGUMENT            # a row pitch under w bpp
        assert call(p, p, 2, 1 << 15, 1 << 15, 1) == _lib.P3D_ERR_ARGUMENT          # 2^31 samples
        assert call(None, None, 0, 12, 12, 3) == _lib.P3D_OK                        # no frame: nothing to read, nothing to do
    decode = lambda c, f, h, w, sub, lq, cq, scratch, n, out, row: lib.p3d_video_jpeg_decode(c, f, h, w, sub, lq, cq, scratch, n, out, 4096, row, None)
    assert decode(p, 1, 16, 16, 2, p, p, p, 4096, p, 48) == _lib.P3D_ERR_ARGUMENT   # 4:2:2 is not served
    assert decode(p, 1, -16, 16, 0, p, p, p, 4096, p, 48) == _lib.P3D_ERR_ARGUMENT
    for k in (0, 5, 6, 7, 9):
        args = [p, 1, 16, 16, 0, p, p, p, 4096, p, 48]
        args[k] = None
        assert decode(*args) == _lib.P3D_ERR_ARGUMENT, k
    assert decode(p, 1, 16, 16, 0, p, p, p, 767, p, 48) == _lib.P3D_ERR_ARGUMENT and b'scratch' in lib.p3d_last_error()      # three planes of 256
    assert decode(p, 1, 16, 16, 1, p, p, p, 383, p, 48) == _lib.P3D_ERR_ARGUMENT    # 256 + 2 x 64
    assert decode(p, 1, 16, 16, 0, p, p, p, 4096, p, 47) == _lib.P3D_ERR_ARGUMENT
    assert decode(None, 0, 16, 16, 0, None, None, None, 0, None, 0) == _lib.P3D_OK
    assert video.launch_count() == n0


def test_python_refuses_bad_arguments():
    Q, video = _q(), _video()
    a = clip(2, 12, 13, 3, seed=23)
    for fn in (Q.error_sums, Q.ssim_sums, Q.compare, Q.difference_map):
        for x, y in ((a, a[:, :, :12]), (a, a[:1]), (a, a[..., 0]), (a.float(), a.float()), (a, a.numpy()), (a[:, :, ::2], a[:, :, ::2]),
                     (a[..., :1], a[..., :1])):
            with pytest.raises(ValueError):
                fn(x, y)
    for out in (torch.zeros([2, 3, 4], dtype=torch.int32), torch.zeros([2, 3, 5], dtype=torch.int64), torch.zeros([2, 3, 8], dtype=torch.int64)[..., ::2]):
        with pytest.raises(ValueError):
            Q.error_sums(a, a, out=out)
    with pytest.raises(ValueError):
        Q.ssim_sums(a, a, out=torch.zeros([2, 3, 4], dtype=torch.int64))
    for kw in ({}, {'psnr': 30.0, 'ssim': 0.9}, {'ssim': 1.5}, {'psnr': -1.0}, {'psnr': 'high'}, {'ssim': float('nan')}, {'psnr': 30.0, 'sample': 0}):
        with pytest.raises(ValueError):
            video.jpeg_quality_for(a, **kw)                                         # one target, and only one
    with pytest.raises(ValueError):
        video.encode_jpeg(a, psnr=30.0, ssim=0.9)
    with pytest.raises(ValueError):
        video.save_avi('never_written.avi', a, psnr=30.0, ssim=0.9)
    tables = video.jpeg_tables(90)
    coefficients = video.jpeg_coefficients(a, tables)
    for bad in (lambda: video.jpeg_decode(coefficients, tables, 12, 40), lambda: video.jpeg_decode(coefficients.int(), tables, 12, 13),
                lambda: video.jpeg_decode(coefficients, (tables[0], tables[1][:63]), 12, 13), lambda: video.jpeg_decode(coefficients, tables, 12, 13, '4:2:2'),
                lambda: video.jpeg_decode(coefficients, tables, 12, 13, out=torch.zeros([2, 12, 13, 4], dtype=torch.uint8)),
                lambda: video.palette_quality(a, torch.zeros([2, 12, 12], dtype=torch.uint8), torch.zeros([4, 3], dtype=torch.uint8))):
        with pytest.raises(ValueError):
            bad()


def test_what_quality_calls_is_declared():
    """tests/test_side_libraries.py scans every module that calls libp3d_video.so for ``video_lib().p3d_*``; the same scan of this one, and of the module
    that holds ``jpeg_decode``."""
    Q, video = _q(), _video()
    called = set(re.findall(r'\bvideo_lib\(\)\.(p3d_\w+)', pathlib.Path(Q.__file__).read_text()))
    assert called == {'p3d_video_error_sums', 'p3d_video_ssim'} and called <= set(video.HEADER.functions)
    from pix2pix3d_amd import _lib, decimate, regions, sketch
    names = ['p3d_video_error_sums', 'p3d_video_ssim', 'p3d_video_jpeg_decode']      # declared by the video header and by no other
    assert all(n in video.HEADER.functions for n in names)
    assert not any(n in header.functions for n in names for header in (_lib.HEADER, regions.HEADER, sketch.HEADER, decimate.HEADER))
    assert 'p3d_video_jpeg_decode' in set(re.findall(r'\bvideo_lib\(\)\.(p3d_\w+)', pathlib.Path(video.jpeg.__file__).read_text()))
