"""Clips, sizes and boxes shared by the resampling tests (test_resample_host.py, test_resample_gpu.py)."""
import numpy as np
import torch

SEPARABLE = ('box', 'bilinear', 'hamming', 'bicubic', 'lanczos')
# ((in width, in height), (out width, out height)): both directions, one axis skipped each way, an axis that shrinks while the other grows, one pixel,
# and the 512 -> 1 Lanczos row of 3073 taps.
SIZE_PAIRS = (((17, 23), (5, 7)), ((17, 23), (40, 31)), ((64, 64), (32, 32)), ((33, 20), (33, 9)), ((20, 33), (7, 33)), ((50, 50), (49, 51)),
              ((8, 8), (64, 64)), ((100, 37), (3, 2)), ((5, 5), (1, 1)), ((512, 3), (1, 3)))
# ((in width, in height), box, (out width, out height)): fractional, integral, fractional at unchanged size, one axis whole
BOXES = (((50, 40), (3.5, 2.25, 41.0, 30.0), (20, 17)), ((50, 40), (4.0, 6.0, 36.0, 38.0), (16, 60)), ((33, 33), (0.5, 0.5, 32.5, 32.5), (33, 33)),
         ((50, 40), (0.0, 10.5, 50.0, 32.25), (50, 13)))
# nearest: ((in width, in height), (out width, out height)); 512 -> 300 and 1000 -> 513 are where the closed form fails
NEAREST_PAIRS = (((17, 23), (5, 7)), ((17, 23), (40, 31)), ((512, 4), (300, 4)), ((1000, 999), (513, 257)), ((8, 8), (64, 64)), ((100, 37), (3, 2)),
                 ((5, 5), (1, 1)), ((50, 50), (49, 51)))
MODES = {'L': 1, 'RGB': 3, 'RGBX': 4}


def uniform_clip(f, h, w, bpp, seed=0):
    """uint8 [f, h, w, bpp] ([f, h, w] for bpp 1) of uniform noise."""
    a = np.random.default_rng(seed).integers(0, 256, size=(f, h, w, bpp), dtype=np.uint8)
    return torch.from_numpy(a[..., 0] if bpp == 1 else a)


def binary_clip(f, h, w, bpp, seed=0):
    """uint8 [f, h, w, bpp] ([f, h, w] for bpp 1) of 0 / 255 noise: the bicubic and Lanczos overshoots reach both clamps."""
    a = np.random.default_rng(seed).integers(0, 2, size=(f, h, w, bpp), dtype=np.uint8) * np.uint8(255)
    return torch.from_numpy(a[..., 0] if bpp == 1 else a)


def label_clip(f, h, w, classes=7, seed=0):
    """uint8 [f, h, w] of class ids that are not consecutive, so that a blended value would not be a class."""
    return torch.from_numpy((np.random.default_rng(seed).integers(0, classes, size=(f, h, w), dtype=np.uint8) * np.uint8(37)))


def pil_image(frame, mode):
    """A PIL image of ``mode`` ('L', 'RGB', 'RGBX') of one frame uint8 [h, w(, bpp)]."""
    from PIL import Image
    a = np.ascontiguousarray(frame.numpy())
    h, w = a.shape[:2]
    return Image.frombytes(mode, (w, h), a.tobytes())


def pil_resize(frame, mode, size, filter, box=None):
    """uint8 [oh, ow(, bpp)]: PIL's resize of one frame."""
    from PIL import Image
    code = {'nearest': Image.NEAREST, 'box': Image.BOX, 'bilinear': Image.BILINEAR, 'hamming': Image.HAMMING, 'bicubic': Image.BICUBIC,
            'lanczos': Image.LANCZOS}[filter]
    out = pil_image(frame, mode).resize(size, code, box=box)
    a = np.frombuffer(out.tobytes(), dtype=np.uint8).reshape((size[1], size[0]) + tuple(frame.shape[2:]))
    return torch.from_numpy(a.copy())


def golden_cases():
    """name -> (frame, mode, size, filter, box): the cases recorded in tests/golden/resample_pil.npz — small, every filter, both directions, the clamps,
    a box, nearest at the size where the closed form fails."""
    cases = {}
    for i, (mode, bpp) in enumerate(MODES.items()):
        for j, filter in enumerate(SEPARABLE):
            clip = (binary_clip if j % 2 else uniform_clip)(1, 23, 17, bpp, seed=100 + 10 * i + j)[0]
            cases[f'{mode}_{filter}_down'] = (clip, mode, (5, 7), filter, None)
            cases[f'{mode}_{filter}_up'] = (clip, mode, (40, 31), filter, None)
    for j, filter in enumerate(SEPARABLE):
        cases[f'box_{filter}'] = (uniform_clip(1, 40, 50, 3, seed=200 + j)[0], 'RGB', (20, 17), filter, (3.5, 2.25, 41.0, 30.0))
    cases['binary_bicubic_8_64'] = (binary_clip(1, 8, 8, 1, seed=300)[0], 'L', (64, 64), 'bicubic', None)
    cases['binary_lanczos_8_64'] = (binary_clip(1, 8, 8, 1, seed=300)[0], 'L', (64, 64), 'lanczos', None)
    cases['long_row'] = (uniform_clip(1, 3, 512, 1, seed=301)[0], 'L', (1, 3), 'lanczos', None)
    cases['nearest_512_300'] = (uniform_clip(1, 2, 512, 1, seed=302)[0], 'L', (300, 2), 'nearest', None)
    return cases


GOLDEN_NAME = 'resample_pil.npz'


def record_golden(path):
    """Write the golden: for every case of ``golden_cases`` the input, PIL's output and what was asked, with the version of the Pillow that answered."""
    import json
    import PIL
    arrays, asked = {}, {}
    for name, (frame, mode, size, filter, box) in golden_cases().items():
        arrays[f'in_{name}'] = frame.numpy()
        arrays[f'out_{name}'] = pil_resize(frame, mode, size, filter, box).numpy()
        asked[name] = dict(mode=mode, size=list(size), filter=filter, box=None if box is None else list(box))
    np.savez_compressed(path, pillow=np.array(PIL.__version__), asked=np.array(json.dumps(asked)), **arrays)


if __name__ == '__main__':
    import os
    record_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', GOLDEN_NAME))
