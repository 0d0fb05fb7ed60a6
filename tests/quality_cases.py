"""Shared by test_quality_host.py / test_quality_gpu.py: clips with known structure, the SSIM rules of p3d_video.h as a plain-Python loop over windows, an
independent fp64 SSIM with the unquantised Gaussian, and the fp64 inverse DCT."""
import numpy as np
import torch

from video_cases import noise_frames

WINDOW = (1, 8, 37, 112, 218, 272, 218, 112, 37, 8, 1)      # p3d_video.h's literals, typed again: the tests compare them with the formula
C1, C2 = round(6.5025 * 2 ** 40), round(58.5225 * 2 ** 40)
# What ``jpeg_decode`` may lose against PIL's decode of the same stream, in dB of PSNR against the source: the worst gap measured over every picture of
# jpeg_cases.PICTURES, both subsamplings, qualities 50 and 90 (0.0141 dB, 'below one MCU' at 4:2:0 and quality 50; most cases gain) plus 0.05 dB.  It
# stands beside the 0.25 dB that test_video_jpeg_host.py grants the encoder against PIL's.
DECODE_MARGIN_DB = 0.0141 + 0.05


def clip(f, h, w, bpp, seed):
    """uint8 [f, h, w, bpp] ([f, h, w] for bpp = 1): smooth ramps plus noise, so that windows differ and no moment is degenerate."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = (3 * x + 5 * y)[None, :, :, None] + 40 * np.arange(bpp)[None, None, None, :] + 17 * np.arange(f)[:, None, None, None]
    a = (base + rng.integers(-30, 31, size=[f, h, w, bpp])) % 256
    a = torch.from_numpy(a.astype(np.uint8))
    return a[..., 0] if bpp == 1 else a


def disturbed(a, seed, amplitude=12):
    """``a`` with noise of +-amplitude on most samples, some left alone, a few pushed to an extreme."""
    rng = np.random.default_rng(seed)
    n = rng.integers(-amplitude, amplitude + 1, size=tuple(a.shape))
    n[rng.random(tuple(a.shape)) < 0.2] = 0
    out = (a.numpy().astype(np.int64) + n).clip(0, 255)
    out[rng.random(tuple(a.shape)) < 0.01] = 255
    return torch.from_numpy(out.astype(np.uint8))


def checkerboard(f, h, w, bpp, cell=1):
    """The extreme pair: a board of 0 and 255 and its complement — means equal, covariance as negative as it gets."""
    y, x = np.mgrid[0:h, 0:w]
    on = (((y // cell + x // cell) % 2) * 255).astype(np.uint8)
    a = torch.from_numpy(np.broadcast_to(on[None, :, :, None], [f, h, w, bpp]).copy())
    a = a[..., 0] if bpp == 1 else a
    return a, 255 - a


def in_canvas(t, pad=(9, 19), frame_step=2):
    """``t`` as every ``frame_step``-th frame and a window of a larger canvas filled with other bytes: the same values, other pitches."""
    f, h, w = t.shape[:3]
    canvas = torch.full([f * frame_step, h + pad[0] + 10, w + pad[1] + 13] + list(t.shape[3:]), 77, dtype=torch.uint8, device=t.device)
    view = canvas[::frame_step, pad[0]:pad[0] + h, pad[1]:pad[1] + w]
    view.copy_(t)
    return view


def ssim_loop(a, b):
    """(sum of contributions, windows) per frame and channel, lists [F][bpp][2], by the header's rules in plain Python integers and floats: one window at a
    time, the 121 weights as the outer product of WINDOW."""
    a, b = a.numpy().astype(np.int64), b.numpy().astype(np.int64)
    if a.ndim == 3:
        a, b = a[..., None], b[..., None]
    f, h, w, bpp = a.shape
    out = [[[0, 0] for _ in range(bpp)] for _ in range(f)]
    for i in range(f):
        for c in range(bpp):
            for y0 in range(h - 10):
                for x0 in range(w - 10):
                    A = B = pxx = pyy = pxy = 0
                    for dy in range(11):
                        for dx in range(11):
                            wgt, x, y = WINDOW[dy] * WINDOW[dx], int(a[i, y0 + dy, x0 + dx, c]), int(b[i, y0 + dy, x0 + dx, c])
                            A, B, pxx, pyy, pxy = A + wgt * x, B + wgt * y, pxx + wgt * x * x, pyy + wgt * y * y, pxy + wgt * x * y
                    n1, n2 = 2 * A * B + C1, 2 * ((pxy << 20) - A * B) + C2
                    d1, d2 = A * A + B * B + C1, ((pxx + pyy) << 20) - A * A - B * B + C2
                    assert max(abs(n1), abs(n2), d1, d2) < 2 ** 59 and d1 > 0 and d2 > 0
                    q = (float(n1) * float(n2)) / (float(d1) * float(d2))         # int -> float rounds to nearest even; three fp64 operations
                    out[i][c][0] += round(q * 2.0 ** 32)                          # Python's round: half to even
                    out[i][c][1] += 1
    return out


def ssim_true(a, b):
    """The mean SSIM over windows and channels in fp64 with the TRUE Gaussian (sigma 1.5, normalised over its 11 taps), variances as E[x^2] - E[x]^2: the
    textbook form, independent of the integer rules.  NaN without a window."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.ndim == 3:
        a, b = a[..., None], b[..., None]
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()
    h, w = a.shape[1:3]
    if h < 11 or w < 11:
        return float('nan')

    def blur(q):
        rows = sum(g[k] * q[:, :, k:k + w - 10] for k in range(11))
        return sum(g[k] * rows[:, k:k + h - 10] for k in range(11))
    mx, my = blur(a), blur(b)
    vx, vy, cxy = blur(a * a) - mx * mx, blur(b * b) - my * my, blur(a * b) - mx * my
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    return float((((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))).mean())


def idct_fp64(blocks):
    """fp64 [..., 8, 8] (y, x): the orthonormal inverse DCT of coefficient blocks [..., 8, 8] (v, u), level shift included, nothing rounded or clamped."""
    u, x = np.arange(8.0)[:, None], np.arange(8.0)[None, :]
    t = np.where(u == 0, np.sqrt(0.125), 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)      # t[u][x]
    return t.T @ np.asarray(blocks, dtype=np.float64) @ t + 128


def grey(picture):
    """uint8 [H, W, 3] with R = G = B: the rounded mean of a picture's channels."""
    v = (picture.astype(np.int64).sum(axis=2) + 1) // 3
    return np.repeat(v[:, :, None], 3, axis=2).astype(np.uint8)
