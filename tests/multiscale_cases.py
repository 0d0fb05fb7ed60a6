"""Shared by test_multiscale_host.py / test_multiscale_gpu.py: the pyramid rule and the per-level rules of p3d_video.h ("multi-scale frame quality") as
plain Python loops, the textbook MS-SSIM in float64 (exact Gaussian, unrounded 2 x 2 mean pooling), and the clips both files measure."""
import functools

import numpy as np
import torch

from quality_cases import C1, C2, WINDOW, clip, disturbed

WANG = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def halve_rule(a):
    """numpy uint8 [F, H // 2, W // 2(, bpp)]: (s00 + s01 + s10 + s11 + 2) >> 2 per channel, one output sample at a time."""
    a = np.asarray(a)
    f, h, w = a.shape[:3]
    out = np.zeros((f, h // 2, w // 2) + a.shape[3:], dtype=np.uint8)
    for y in range(h // 2):
        for x in range(w // 2):
            block = a[:, 2 * y:2 * y + 2, 2 * x:2 * x + 2].astype(np.int64)
            out[:, y, x] = (block[:, 0, 0] + block[:, 0, 1] + block[:, 1, 0] + block[:, 1, 1] + 2) >> 2
    return out


def odd_pitch_view(t):
    """``t`` as a window of a larger canvas of other bytes whose row pitch is an ODD number of bytes (and whose first byte is off a dword): the same
    values, and no two rows start at the same alignment."""
    f, h, w = t.shape[:3]
    bpp = t.shape[3] if t.ndim == 4 else 1
    row = (w * bpp + 6) | 1
    frame = (h + 2) * row
    canvas = torch.full([f * frame + 8], 77, dtype=torch.uint8, device=t.device)
    view = canvas.as_strided(tuple(t.shape), (frame, row, bpp, 1)[:t.ndim], 3)
    view.copy_(t)
    return view


SINGLE_LEVEL_SIZES = ((1, 11, 11), (2, 27, 43))        # (F, H, W): one window; 17 x 33 windows, one past the 16 x 32 tile both ways


def single_level_agrees(a, b):
    """``ssim_sums`` equals the q sum and the window count of a one-level ``msssim_sums``, byte for byte, for the clips as they are and as windows of a
    canvas with an odd row pitch — on the device the byte staging of one kernel against the dword staging of the other."""
    from pix2pix3d_amd import multiscale, quality
    for x, y in ((a, b), (odd_pitch_view(a), odd_pitch_view(b)), (a, odd_pitch_view(b))):
        assert x.stride(1) % 2 == 1 or x is a
        one, many = quality.ssim_sums(x, y), multiscale.msssim_sums(x, y, levels=1)
        assert one.dtype == many.dtype == torch.int64 and one.device == many.device == a.device
        assert torch.equal(one, many[:, :, 0, [0, 2]]), (tuple(a.shape), x.stride(), y.stride())
    return one


def msssim_loop(a, b, levels):
    """Lists [F][bpp][levels][3] = (sum of round(q 2^32), sum of round(cs 2^32), windows) by the header's rules in plain Python integers and floats: one
    window at a time with the 121 weights as the outer product of WINDOW, and ``halve_rule`` between the levels."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim == 3:
        a, b = a[..., None], b[..., None]
    f, _, _, bpp = a.shape
    out = [[[[0, 0, 0] for _ in range(levels)] for _ in range(bpp)] for _ in range(f)]
    for k in range(levels):
        h, w = a.shape[1:3]
        assert h >= 11 and w >= 11
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
                        q = (float(n1) * float(n2)) / (float(d1) * float(d2))     # int -> float rounds to nearest even; three fp64 operations
                        cs = float(n2) / float(d2)                                # two conversions, one division
                        cell = out[i][c][k]
                        cell[0], cell[1], cell[2] = cell[0] + round(q * 2.0 ** 32), cell[1] + round(cs * 2.0 ** 32), cell[2] + 1      # round: half to even
        if k + 1 < levels:
            a, b = halve_rule(a), halve_rule(b)
    return out


def msssim_true(a, b, levels=5, weights=None):
    """The textbook MS-SSIM in float64, independent of the integer rules: the TRUE Gaussian (sigma 1.5, normalised over its 11 taps), variances as
    E[x^2] - E[x]^2, K1 = 0.01, K2 = 0.03, the same valid windows, the pyramid by UNROUNDED 2 x 2 means (an odd last row or column dropped).  Per frame
    and channel prod_{k < L - 1} max(mean cs_k, 0)^(w_k) * max(mean (l cs)_(L-1), 0)^(w_(L-1)); the mean of those over frames and channels."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.ndim == 3:
        a, b = a[..., None], b[..., None]
    weights = np.asarray(WANG[:levels]) / sum(WANG[:levels]) if weights is None else np.asarray(weights, dtype=np.float64)
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    g /= g.sum()
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    result = np.ones(a.shape[:1] + a.shape[3:])
    for k in range(levels):
        h, w = a.shape[1:3]

        def blur(q):
            rows = sum(g[t] * q[:, :, t:t + w - 10] for t in range(11))
            return sum(g[t] * rows[:, t:t + h - 10] for t in range(11))
        mx, my = blur(a), blur(b)
        vx, vy, cxy = blur(a * a) - mx * mx, blur(b * b) - my * my, blur(a * b) - mx * my
        cs = (2 * cxy + c2) / (vx + vy + c2)
        term = cs if k + 1 < levels else cs * (2 * mx * my + c1) / (mx * mx + my * my + c1)
        result = result * np.maximum(term.mean(axis=(1, 2)), 0.0) ** weights[k]
        if k + 1 < levels:
            a, b = (0.25 * (t[:, 0:h // 2 * 2:2, 0:w // 2 * 2:2] + t[:, 0:h // 2 * 2:2, 1:w // 2 * 2:2] + t[:, 1:h // 2 * 2:2, 0:w // 2 * 2:2]
                            + t[:, 1:h // 2 * 2:2, 1:w // 2 * 2:2]) for t in (a, b))
    return float(result.mean())


def smooth_pair(f, h, w, bpp, seed):
    """A smooth gradient clip and the same clip blurred along x by a [1 2 1] / 4 kernel and shifted in level: the loss that shows at coarse scales."""
    rng = np.random.default_rng(seed)
    i, y, x, c = np.arange(f)[:, None, None, None], np.arange(h)[None, :, None, None], np.arange(w)[None, None, :, None], np.arange(bpp)[None, None, None, :]
    base = 96 + 60 * np.sin(x / 23.0 + 0.3 * c) + 50 * np.cos(y / 17.0 + 0.5 * i)
    a = np.clip(base + rng.normal(0, 3, size=[f, h, w, bpp]), 0, 255).round()
    padded = np.pad(a, ((0, 0), (0, 0), (1, 1), (0, 0)), mode='edge')
    b = np.clip((padded[:, :, :-2] + 2 * padded[:, :, 1:-1] + padded[:, :, 2:]) / 4 + 3, 0, 255).round()
    a, b = torch.from_numpy(a.astype(np.uint8)), torch.from_numpy(b.astype(np.uint8))
    return (a[..., 0], b[..., 0]) if bpp == 1 else (a, b)


@functools.lru_cache(maxsize=None)
def pairs(h=177, w=190):
    """name -> (a, b): the clips of the float comparison — random, a smooth gradient, ``disturbed``, and JPEG-degraded (the package's own coder, CPU tensors).
    Made once a size and shared: no test writes to them."""
    from pix2pix3d_amd import video
    rng = np.random.default_rng(5)
    noise_a, noise_b = (torch.from_numpy(rng.integers(0, 256, size=[1, h, w, 3], dtype=np.uint8)) for _ in range(2))
    base = clip(2, h, w, 3, seed=6)
    smooth = smooth_pair(1, h, w, 3, seed=7)
    return {'random': (noise_a, noise_b), 'smooth': smooth, 'disturbed': (base, disturbed(base, seed=8)),
            'jpeg q30 4:2:0': (video.jpeg_reconstruct(smooth[0], 30, '4:2:0'), smooth[0]),
            'jpeg q75 4:4:4': (video.jpeg_reconstruct(base, 75, '4:4:4'), base)}
