"""Shared by test_video_jpeg_host.py / test_video_jpeg_gpu.py: pictures with known structure, a JPEG segment parser, a first-principles entropy coder
(a loop, bit by bit) and PIL's own encoder as the yardstick for quality."""
import io

import numpy as np
import torch

from video_cases import noise_frames

SUBSAMPLINGS = ('4:4:4', '4:2:0')
PIL_SUBSAMPLING = {'4:4:4': 0, '4:2:0': 2}


def _gradient_with_a_flat_patch(h=37, w=53):
    """Smooth colour ramps, +-6 grey levels of noise, and a flat patch in the middle."""
    rng = np.random.default_rng(31)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.stack([255 * x / (w - 1), 255 * y / (h - 1), 127.5 + 127.5 * np.sin(6.0 * (x + y) / (h + w))], axis=2)
    a += rng.integers(-6, 7, size=a.shape)
    a[10:24, 14:36] = (201, 17, 94)
    return a.clip(0, 255).astype(np.uint8)


def _checkerboard(h=16, w=64):
    y, x = np.mgrid[0:h, 0:w]
    on = ((y // 8 + x // 8) % 2).astype(np.uint8)
    return np.stack([255 * on, 255 * on, 255 * on], axis=2).astype(np.uint8)


def _pictures():
    flat = np.empty([20, 20, 3], dtype=np.uint8)
    flat[:] = (201, 17, 94)
    return {'single pixel': np.array([[[37, 150, 211]]], dtype=np.uint8),
            'below one MCU': noise_frames(1, 7, 9, seed=32)[0].numpy() // 4 + 90,
            'flat': flat,
            'gradient': _gradient_with_a_flat_patch(),
            'noise': noise_frames(1, 24, 40, seed=33)[0].numpy(),
            'checkerboard': _checkerboard()}


PICTURES = _pictures()                               # name -> uint8 [H, W, 3]; read only


def frames_of(name):
    return torch.from_numpy(PICTURES[name])[None]


def split_jpeg(stream):
    """(segments, scan): the (marker, payload) pairs from SOI to SOS, and the entropy-coded bytes between SOS and EOI."""
    assert stream[:2] == b'\xff\xd8' and stream[-2:] == b'\xff\xd9', 'SOI / EOI'
    at, segments = 2, []
    while True:
        assert stream[at] == 0xFF, f'a marker at {at}'
        marker, size = stream[at + 1], int.from_bytes(stream[at + 2:at + 4], 'big')
        segments.append((marker, stream[at + 4:at + 2 + size]))
        at += 2 + size
        if marker == 0xDA:
            return segments, stream[at:-2]


def tables_of(stream):
    """(quantisation tables id -> 64 values in the file's (zigzag) order, Huffman tables Tc << 4 | Th -> (BITS, HUFFVAL)) parsed from the bytes."""
    dqt, dht = {}, {}
    for marker, p in split_jpeg(stream)[0]:
        while marker == 0xDB and p:
            assert p[0] >> 4 == 0, '8-bit tables'
            dqt[p[0] & 15], p = tuple(p[1:65]), p[65:]
        while marker == 0xC4 and p:
            n = sum(p[1:17])
            dht[p[0]], p = (tuple(p[1:17]), tuple(p[17:17 + n])), p[17 + n:]
    return dqt, dht


def pil_jpeg(picture, quality, subsampling):
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(picture).save(out, 'JPEG', quality=quality, subsampling=PIL_SUBSAMPLING[subsampling])
    return out.getvalue()


def decode(stream):
    from PIL import Image
    with Image.open(io.BytesIO(stream)) as im:
        im.load()
        assert im.mode == 'RGB' and im.format == 'JPEG'
        return np.asarray(im).copy()


def psnr(a, b):
    err = ((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2).mean()
    return np.inf if err == 0 else 10 * np.log10(255.0 ** 2 / err)


# ---- the entropy coder from first principles ---------------------------------------------------------------------------------------------------
def canonical_codes(bits, values):
    """symbol -> (code, length) of a DHT's BITS / HUFFVAL: codes of one length count up, and the next length continues from twice the last code plus two."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[values[k]] = (code, length)
            code, k = code + 1, k + 1
        code *= 2
    return codes


def reference_scan(blocks, bpm, restart, tables):
    """(bytes, bits of every interval) of one frame's ``blocks`` (rows of 64 ints in zigzag order, MCU after MCU); ``tables``: four (BITS, HUFFVAL) in
    the order DC luma, DC chroma, AC luma, AC chroma.  Plain Python: one bit at a time."""
    codes = [canonical_codes(*t) for t in tables]
    out, interval_bits = bytearray(), []
    n_mcu = len(blocks) // bpm
    n_intervals = -(-n_mcu // restart)

    def put(bits, value, n):
        for b in range(n - 1, -1, -1):
            bits.append((value >> b) & 1)

    def put_value(bits, code_table, symbol, v, size):
        put(bits, *code_table[symbol])
        if size:
            put(bits, v if v > 0 else v + (1 << size) - 1, size)
    for i in range(n_intervals):
        bits, pred = [], [0, 0, 0]
        for m in range(i * restart, min((i + 1) * restart, n_mcu)):
            for k in range(bpm):
                comp = k if bpm == 3 else max(k - 3, 0)
                dc_codes, ac_codes = codes[1 if comp else 0], codes[3 if comp else 2]
                block = [int(v) for v in blocks[m * bpm + k]]
                diff = block[0] - pred[comp]
                pred[comp] = block[0]
                put_value(bits, dc_codes, abs(diff).bit_length(), diff, abs(diff).bit_length())
                run = 0
                for v in block[1:]:
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        put(bits, *ac_codes[0xF0])
                        run -= 16
                    put_value(bits, ac_codes, run << 4 | abs(v).bit_length(), v, abs(v).bit_length())
                    run = 0
                if run:
                    put(bits, *ac_codes[0x00])
        interval_bits.append(len(bits))
        while len(bits) % 8:
            bits.append(1)
        for j in range(0, len(bits), 8):
            byte = int(''.join(map(str, bits[j:j + 8])), 2)
            out.append(byte)
            if byte == 0xFF:
                out.append(0)
        if i != n_intervals - 1:
            out += bytes([0xFF, 0xD0 + i % 8])
    return bytes(out), interval_bits


def random_coefficients(f, n_mcu, bpm, seed, density=0.2):
    """int16 [f, n_mcu, bpm, 64]: sparse blocks with long zero runs, both signs and every size category — DC over its whole range, AC up to +-1023."""
    rng = np.random.default_rng(seed)
    shape = [f, n_mcu, bpm, 64]
    magnitude = (2.0 ** rng.uniform(0, 10, size=shape)).astype(np.int64).clip(1, 1023)
    c = np.where(rng.random(shape) < density, magnitude * rng.choice([-1, 1], size=shape), 0)
    c[..., 0] = rng.integers(-1024, 1024, size=shape[:3])
    c[:, ::3, :, 40:] = 0                                                          # runs to the end of the block
    c[:, 1::5, :, 1:62] = 0                                                        # ... and runs past 16, 32 and 48 zeros
    return torch.from_numpy(c.astype(np.int16))
