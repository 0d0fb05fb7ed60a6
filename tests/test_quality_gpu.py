"""Frame quality on the device (csrc/video/video_quality.hip, the decode kernels of video_jpeg.hip): the kernels' bytes against the
CPU formulations — integer equality, the float map bit for bit — on every path the kernels have: 1, 3 and 4 bytes a pixel, frames and windows read in place,
partial tiles both ways, one window, none, accumulation; the decoder at both subsamplings, at sizes under and past an MCU, on the clamps and into a pitched
output; the quality search on the device against the host's; and the whole path at real size."""
import io

import numpy as np
import pytest
import torch

from jpeg_cases import SUBSAMPLINGS, psnr
from quality_cases import DECODE_MARGIN_DB, checkerboard, clip, disturbed
from video_cases import gradient_frames, noise_frames

pytestmark = pytest.mark.gpu


def _q():
    from pix2pix3d_amd import quality
    return quality


def _launches(fn, expected):
    from pix2pix3d_amd import video
    n0 = video.launch_count()
    out = fn()
    assert video.launch_count() == n0 + expected, (video.launch_count() - n0, expected)
    return out


def _same_sums(a, b, launches=(1, 1)):
    """Both kernels on the device pair against the formulations on its host copy; returns the device sums."""
    Q = _q()
    assert a.is_cuda and b.is_cuda
    error = _launches(lambda: Q.error_sums(a, b), launches[0])
    ssim, maps = _launches(lambda: Q.ssim_sums(a, b, maps=True), launches[1])
    host_ssim, host_maps = Q.ssim_sums(a.cpu(), b.cpu(), maps=True)
    assert error.is_cuda and error.cpu().tolist() == Q.error_sums(a.cpu(), b.cpu()).tolist()
    assert ssim.is_cuda and ssim.cpu().tolist() == host_ssim.tolist()
    assert maps.is_cuda and maps.dtype == torch.float32 and maps.shape == host_maps.shape and torch.equal(maps.cpu().view(torch.int32), host_maps.view(torch.int32))
    return error, ssim


@pytest.mark.parametrize('bpp', [1, 3, 4])
def test_the_sums_equal_the_cpu_formulation_in_place(hip_lib, bpp):
    """Every second frame of six, a 45 x 77 window of a 64 x 96 canvas: 35 x 67 windows, so three tiles each way and partial ones at both ends."""
    canvas_a = clip(6, 64, 96, bpp, seed=40 + bpp).cuda()
    canvas_b = disturbed(clip(6, 64, 96, bpp, seed=40 + bpp), seed=50 + bpp).cuda()
    a, b = canvas_a[::2, 9:54, 11:88], canvas_b[::2, 9:54, 11:88]
    assert not a.is_contiguous() and tuple(a.shape[:3]) == (3, 45, 77)
    error, ssim = _same_sums(a, b)
    assert ssim[:, :, 1].cpu().tolist() == [[35 * 67] * bpp] * 3 and tuple(error.shape) == (3, bpp, 4)
    other = canvas_b.clone()[1::2, 5:50, 3:80]                                      # the two clips need not share their pitches
    _same_sums(a, other)
    m_dev, m_host = _q().compare(a, b), _q().compare(a.cpu(), b.cpu())
    assert m_dev == m_host and 0 < m_dev['ssim'] < 1


def test_one_window_and_none(hip_lib):
    Q = _q()
    a = clip(2, 11, 11, 3, seed=60).cuda()
    b = disturbed(a.cpu(), seed=61).cuda()
    _, ssim = _same_sums(a, b)
    assert ssim[:, :, 1].cpu().tolist() == [[1] * 3] * 2
    a = clip(2, 10, 40, 3, seed=62).cuda()
    b = disturbed(a.cpu(), seed=63).cuda()
    counters = torch.full([2, 3, 2], 5, dtype=torch.int64, device='cuda')
    out, maps = _launches(lambda: Q.ssim_sums(a, b, out=counters, maps=True), 0)
    assert out is counters and bool((counters == 5).all()) and tuple(maps.shape) == (2, 0, 30, 3)
    _same_sums(a, b, launches=(1, 0))


def test_identical_and_anti_correlated_pairs(hip_lib):
    a = clip(2, 30, 41, 3, seed=64).cuda()
    error, ssim = _same_sums(a, a.clone())
    assert not error.any() and ssim.cpu().tolist() == [[[20 * 31 << 32, 20 * 31]] * 3] * 2
    x, y = (t.cuda() for t in checkerboard(1, 13, 12, 3))
    error, ssim = _same_sums(x, y)
    assert int(ssim[0, 0, 0]) < -(6 << 31) and error[0, :, 2].cpu().tolist() == [255] * 3
    x, y = (t.cuda() for t in checkerboard(1, 40, 50, 1, cell=5))
    _same_sums(x, y)
    white, black = torch.full([1, 20, 20, 4], 255, dtype=torch.uint8, device='cuda'), torch.zeros([1, 20, 20, 4], dtype=torch.uint8, device='cuda')
    _same_sums(white, black)


def test_calls_accumulate(hip_lib):
    Q = _q()
    a = clip(3, 23, 37, 3, seed=65).cuda()
    b = disturbed(a.cpu(), seed=66).cuda()
    error, ssim = Q.error_sums(a, b), Q.ssim_sums(a, b)
    once_error, once_ssim = error.clone(), ssim.clone()
    assert Q.error_sums(a, b, out=error) is error and Q.ssim_sums(a, b, out=ssim) is ssim
    expected = 2 * once_error
    expected[..., 2] = once_error[..., 2]                                          # a maximum stays
    assert torch.equal(error, expected) and torch.equal(ssim, 2 * once_ssim)
    total = Q.Quality('cuda')
    total.add(a, b)
    total.add(a[:1, :12], b[:1, :12])
    host = Q.Quality('cpu')
    host.add(a.cpu(), b.cpu())
    host.add(a[:1, :12].cpu(), b[:1, :12].cpu())
    assert total.result() == host.result() and total.result()['frames'] == 4


def test_no_frames_launch_nothing(hip_lib):
    Q = _q()
    a = torch.empty([0, 16, 16, 3], dtype=torch.uint8, device='cuda')
    error = _launches(lambda: Q.error_sums(a, a), 0)
    ssim = _launches(lambda: Q.ssim_sums(a, a), 0)
    assert error.is_cuda and tuple(error.shape) == (0, 3, 4) and tuple(ssim.shape) == (0, 3, 2)
    empty = torch.empty([2, 0, 16, 3], dtype=torch.uint8, device='cuda')
    assert not _launches(lambda: Q.error_sums(empty, empty), 0).any()


# ---- the decoder ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
@pytest.mark.parametrize('h, w', [(16, 16), (17, 23), (40, 56)])
def test_the_decoder_equals_the_cpu_formulation(hip_lib, h, w, subsampling):
    from pix2pix3d_amd import video
    frames = torch.cat([gradient_frames(1, h, w, seed=70), noise_frames(1, h, w, seed=71)])
    for quality in (10, 95):
        tables = video.jpeg_tables(quality)
        coefficients = video.jpeg_coefficients(frames, tables, subsampling)
        shown = _launches(lambda: video.jpeg_decode(coefficients.cuda(), tables, h, w, subsampling), 2)
        assert shown.is_cuda and torch.equal(shown.cpu(), video.jpeg_decode(coefficients, tables, h, w, subsampling))
        assert torch.equal(_launches(lambda: video.jpeg_reconstruct(frames.cuda(), quality, subsampling), 3).cpu(), shown.cpu())


@pytest.mark.parametrize('subsampling', SUBSAMPLINGS)
def test_the_decoder_clamps_and_writes_in_place(hip_lib, subsampling):
    from pix2pix3d_amd import video
    h, w = 37, 41
    _, n_mcu, bpm, _ = video.jpeg_layout(h, w, subsampling)
    rng = np.random.default_rng(72)
    extreme = torch.from_numpy((rng.integers(0, 2, size=[2, n_mcu, bpm, 64]) * 2046 - 1023).astype(np.int16))
    tables = (torch.full([64], 255, dtype=torch.uint8),) * 2
    expected = video.jpeg_decode(extreme, tables, h, w, subsampling)
    assert int(expected.min()) == 0 and int(expected.max()) == 255
    canvas = torch.full([4, 50, 60, 3], 9, dtype=torch.uint8, device='cuda')
    view = canvas[::2, 5:5 + h, 7:7 + w]
    assert video.jpeg_decode(extreme.cuda(), tables, h, w, subsampling, out=view) is view and torch.equal(view.cpu(), expected)
    canvas[::2, 5:5 + h, 7:7 + w] = 9
    assert bool((canvas == 9).all())                                                # nothing around the window was written
    assert _launches(lambda: video.jpeg_decode(extreme[:0].cuda(), tables, h, w, subsampling), 0).shape == (0, h, w, 3)


# ---- from a target to a setting ----------------------------------------------------------------------------------------------------------------------
def test_the_quality_search_agrees_with_the_host(hip_lib):
    from pix2pix3d_amd import video
    frames = gradient_frames(4, 64, 64, seed=73, noise=8)
    for target in ({'psnr': 34.0}, {'ssim': 0.88}, {'psnr': 99.0}):
        on_device, on_host = video.jpeg_quality_for(frames.cuda(), **target), video.jpeg_quality_for(frames, **target)
        assert on_device == on_host, (target, on_device[0], on_host[0])
    assert on_host[::2] == (100, False) and video.jpeg_quality_for(frames, psnr=34.0)[2]


def test_save_avi_meets_its_target_as_pil_decodes_it(hip_lib, tmp_path):
    from PIL import Image
    from pix2pix3d_amd import video
    frames = gradient_frames(4, 64, 64, seed=74, noise=8)
    streams = video.save_avi(tmp_path / 'a.avi', frames.cuda(), psnr=34.0)
    quality, metrics, met = video.jpeg_quality_for(frames, psnr=34.0)
    assert met and streams == video.encode_jpeg(frames, quality) == video.read_avi(tmp_path / 'a.avi')[0]
    decoded = np.stack([np.asarray(Image.open(io.BytesIO(s)).convert('RGB')) for s in streams])
    print(f'save_avi(psnr=34): quality {quality}, measured {metrics["psnr"]:.4f} dB, PIL decodes {psnr(decoded, frames.numpy()):.4f} dB')
    assert psnr(decoded, frames.numpy()) >= 34.0 - DECODE_MARGIN_DB


def test_generate_video_meets_an_ssim_target_at_real_size(hip_lib, tmp_path):
    from model_cases import build_generator
    from pix2pix3d_amd import views, video
    G = build_generator('seg2cat', 'cuda', depth=(64, 64))
    ws = torch.randn(1, G.backbone.num_ws, G.w_dim, generator=torch.Generator().manual_seed(41)).cuda()
    n0 = video.launch_count()
    runs = []
    for tag in ('a', 'b'):
        torch.manual_seed(3)
        runs.append(views.generate_video(G, ws, 'seg2cat', str(tmp_path / f'{tag}.avi'), n_frames=4, views_per_step=4, format='avi', ssim=0.95))
    assert video.launch_count() > n0 and (tmp_path / 'a.avi').stat().st_size > 0
    quality, metrics, met = runs[0]['jpeg_quality']
    print(f'generate_video(ssim=0.95): quality {quality}, ssim {metrics["ssim"]:.5f}, psnr {metrics["psnr"]:.3f} dB, met {met}')
    assert runs[0]['image'].is_cuda and tuple(runs[0]['image'].shape[1:3]) == (512, 512) and 1 <= quality <= 100
    assert met == (metrics['ssim'] >= 0.95) and (met or quality == 100)
    assert torch.equal(runs[0]['image'], runs[1]['image']) and runs[0]['jpeg_quality'] == runs[1]['jpeg_quality']
    assert (tmp_path / 'a.avi').read_bytes() == (tmp_path / 'b.avi').read_bytes()
    assert video.read_avi(tmp_path / 'a.avi')[0] == video.encode_jpeg(runs[0]['image'], quality)
