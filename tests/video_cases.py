"""Shared by test_video_host.py / test_video_gpu.py: frames with known structure for pix2pix3d_amd.video."""
import numpy as np
import torch


def gradient_frames(f, h, w, seed=0, noise=3, drift=2 * np.pi / 120):
    """uint8 [f, h, w, 3]: smooth colour gradients plus ``noise`` grey levels of noise, as consecutive frames of a 60 fps turntable are to a colour quantiser:
    red and green follow a diagonal wave that travels by ``drift`` radians a frame (1 / 120 of its period: a 120-frame turn), blue is a static vertical
    ramp.  Every frame differs from the one before."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty([f, h, w, 3])
    for i in range(f):
        t = 6.0 * (x + y) / (h + w) + drift * i
        out[i, ..., 0] = 127.5 + 127.5 * np.sin(t)
        out[i, ..., 1] = 127.5 + 127.5 * np.sin(t + 2.0)
        out[i, ..., 2] = 255 * y / max(h - 1, 1)
    out += rng.integers(-noise, noise + 1, size=out.shape)
    return torch.from_numpy(out.clip(0, 255).astype(np.uint8))


def noise_frames(f, h, w, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=[f, h, w, 3], dtype=np.uint8))


def every_bin_once():
    """uint8 [1, 256, 128, 3]: 32768 pixels, one in every bin, in a shuffled order and at a random place inside the bin's 8 x 8 x 8 cell."""
    rng = np.random.default_rng(5)
    bins = rng.permutation(32768)
    rgb = np.stack([bins >> 10, (bins >> 5) & 31, bins & 31], axis=1) * 8 + rng.integers(0, 8, size=[32768, 3])
    return torch.from_numpy(rgb.astype(np.uint8).reshape(1, 256, 128, 3))


def decode_gif(path):
    """uint8 [F, H, W, 3]: every frame of a GIF as PIL composes it."""
    from PIL import Image
    with Image.open(path) as im:
        frames = []
        for i in range(im.n_frames):
            im.seek(i)
            frames.append(np.asarray(im.convert('RGB')).copy())
    return np.stack(frames)


def psnr(a, b):
    err = (np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2
    return 10 * np.log10(255.0 ** 2 / err.mean())
