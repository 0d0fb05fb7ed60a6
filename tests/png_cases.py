"""Shared by test_video_png_host.py / test_video_png_gpu.py: pictures with known structure for the PNG stages of pix2pix3d_amd.video, and first-principles
formulations to hold them against — the adaptive row filter one byte at a time, the token rule as a loop over runs, a Huffman code by ``heapq``, PIL as the
decoder.  Everything here is made once and only read."""
import heapq
import io

import numpy as np
import torch

from video_cases import noise_frames

MODES = ('L', 'LA', 'RGB', 'RGBA', 'P', 'I;16')
BPP = {'L': 1, 'LA': 2, 'RGB': 3, 'RGBA': 4, 'P': 1, 'I;16': 2}


# ---- pictures ------------------------------------------------------------------------------------------------------------------------------------
def filter_pictures(h=24, w=40):
    """name -> uint8 [h, w, 3]: the five kinds of rows the adaptive filter must tell apart."""
    rng = np.random.default_rng(71)
    y, x = np.mgrid[0:h, 0:w]
    one = np.ones(3, dtype=np.int64)
    return {'horizontal ramp': ((5 * x)[..., None] * one) & 255,                    # rows repeat: Up; the first row: Sub
            'vertical ramp': ((7 * y)[..., None] * one) & 255,                      # constant rows: Paeth, whose first pixel takes the byte above (the first row, all zeros: None)
            'diagonal ramp': np.stack([x + 7 * y, 7 * x + y, 3 * x + 3 * y], axis=2) & 255,      # steep across in one channel, steep down in the next: Paeth
            'noise': rng.integers(0, 256, size=[h, w, 3]),
            'gradient and noise': (2 * x + 3 * y)[..., None] * one + rng.integers(-9, 10, size=[h, w, 3]) + 20}      # two noisy neighbours: their Average


def picture_frames(name):
    return torch.from_numpy(filter_pictures()[name].clip(0, 255).astype(np.uint8))[None]


def mode_frames(mode, f=2, h=13, w=37, seed=72):
    """(frames, palette or None) of ``mode``: smooth ramps with a little noise and a flat patch — rows that compress, filters that differ."""
    rng = np.random.default_rng(seed + MODES.index(mode))
    bpp = BPP[mode]
    y, x = np.mgrid[0:h, 0:w]
    if mode == 'P':
        a = ((x // 5 + y // 3 + np.arange(f)[:, None, None]) % 19).astype(np.uint8)
        a[:, 4:9, 10:30] = 7
        return torch.from_numpy(a), torch.from_numpy(rng.integers(0, 256, size=[19, 3], dtype=np.uint8))
    a = np.stack([(3 + c) * x + (2 + c) * y + 11 * c for c in range(bpp)], axis=2)[None] + 5 * np.arange(f)[:, None, None, None]
    a = a + rng.integers(-2, 3, size=a.shape)
    a[:, 4:9, 10:30] = 77
    a = (a & 255).astype(np.uint8)
    return torch.from_numpy(a[..., 0] if bpp == 1 else a), None


def decode(stream, mode):
    """The file's pixels as the mode's input array: PIL is the decoder."""
    from PIL import Image
    with Image.open(io.BytesIO(stream)) as im:
        im.load()
        assert im.format == 'PNG'
        if mode == 'I;16':
            assert im.mode in ('I;16', 'I;16B', 'I'), im.mode
            v = np.asarray(im).astype(np.int64)
            return np.stack([v >> 8, v & 255], axis=2).astype(np.uint8)
        assert im.mode == mode, (im.mode, mode)
        return np.asarray(im).copy()


def decode_palette(stream):
    from PIL import Image
    with Image.open(io.BytesIO(stream)) as im:
        return np.asarray(im.convert('RGB')).copy()


def decode_apng(path):
    """(frames in the file's own mode converted to arrays, durations, loop) as PIL composes them."""
    from PIL import Image
    with Image.open(path) as im:
        frames, durations = [], []
        for i in range(im.n_frames):
            im.seek(i)
            frames.append(np.asarray(im.convert('RGB') if im.mode == 'P' else im).copy())
            durations.append(im.info.get('duration'))
        return frames, durations, im.info.get('loop')


# ---- the filter, one byte at a time ------------------------------------------------------------------------------------------------------------------
def reference_filter_row(cur, prev, bpp):
    """(type, residual bytes) of one row of ints under the adaptive rule: the smallest sum of |residual as int8|, the lowest type on a tie."""
    best = None
    for kind in range(5):
        out = []
        for i, x in enumerate(cur):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if kind == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            else:
                pred = (0, a, b, (a + b) // 2)[kind]
            out.append((x - pred) % 256)
        cost = sum(r if r < 128 else 256 - r for r in out)
        if best is None or cost < best[0]:
            best = (cost, kind, out)
    return best[1], best[2]


def reference_filter(frame, bpp):
    """uint8 [H, 1 + W bpp] of ONE frame [H, W(, bpp)] by ``reference_filter_row``."""
    rows = np.asarray(frame).reshape(frame.shape[0], -1).astype(np.int64).tolist()
    prev, out = [0] * len(rows[0]), []
    for cur in rows:
        kind, residuals = reference_filter_row(cur, prev, bpp)
        out.append([kind] + residuals)
        prev = cur
    return np.array(out, dtype=np.uint8)


# ---- tokens, as the stream definition words them ----------------------------------------------------------------------------------------------------
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)


def reference_tokens(segment):
    """[('lit', byte) | ('match', length)] of one segment's bytes: maximal runs; a literal, then greedy matches of min(m, 258) while m >= 3, then literals."""
    tokens, i = [], 0
    while i < len(segment):
        n = 1
        while i + n < len(segment) and segment[i + n] == segment[i]:
            n += 1
        tokens.append(('lit', segment[i]))
        m = n - 1
        while m >= 3:
            tokens.append(('match', min(m, 258)))
            m -= min(m, 258)
        tokens += [('lit', segment[i])] * m
        i += n
    return tokens


def reference_stats(segment):
    """The 290 numbers ``png_counts`` reports for one segment, from ``reference_tokens`` and the Adler-32 definition."""
    stats = [0] * 290
    for kind, v in reference_tokens(segment):
        if kind == 'lit':
            stats[v] += 1
        else:
            k = max(j for j, base in enumerate(LENGTH_BASE) if base <= v)
            stats[257 + k] += 1
            stats[286] += LENGTH_EXTRA[k]
            stats[287] += 1
    size = len(segment)
    stats[288] = sum(segment) % 65521
    stats[289] = sum((size - i) * b for i, b in enumerate(segment)) % 65521
    return stats


# ---- Huffman by heapq ---------------------------------------------------------------------------------------------------------------------------------
def huffman_lengths(counts):
    """symbol -> depth in a plain Huffman tree of the used symbols (two or more)."""
    heap = [(int(c), s, (s,)) for s, c in enumerate(counts) if c]
    depth = {s: 0 for _, s, _ in heap}
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    return depth


def fibonacci_counts(n=30):
    counts = [1, 1]
    while len(counts) < n:
        counts.append(counts[-1] + counts[-2])
    return counts


_fibonacci = {}


def fibonacci_frame(w=2048):
    """uint8 [1, H, w] for mode 'L' and filter 0: the byte values 1 .. 30 as often as the Fibonacci numbers say, shuffled, after a head of the two rarest values
    in turn, 64 times — 15-bit codes one after the other, 15 bits apart, so that they start at every bit of a 32-bit word — and filled up to whole rows with the
    most frequent value."""
    if w not in _fibonacci:
        counts = fibonacci_counts()
        body = np.repeat(np.arange(1, 31), counts)
        np.random.default_rng(73).shuffle(body)
        head = np.tile([1, 2], 64)
        n = head.shape[0] + body.shape[0]
        h = -(-n // w)
        _fibonacci[w] = torch.from_numpy(np.concatenate([head, body, np.full(h * w - n, 30)]).astype(np.uint8).reshape(1, h, w))
    return _fibonacci[w]


def crafted_rows():
    """uint8 [5, 1, w] for mode 'L' and filter 0: one row each, whose long run leaves m = 258, 259, 260, 261 and 2 * 258 + 2 bytes after its first literal (every
    way a run can end), between two other bytes.  The filter type byte 0 stands before each row, so the run's value is not 0."""
    w = 3 + 2 * 258 + 2 + 3
    rows = np.zeros([5, 1, w], dtype=np.uint8)
    for i, m in enumerate((258, 259, 260, 261, 2 * 258 + 2)):
        rows[i, 0] = np.arange(w) % 251 + 1                                       # no two neighbours equal
        rows[i, 0, 3:3 + m + 1] = 253
        rows[i, 0, 3 + m + 1] = 9
    return torch.from_numpy(rows)


def chunk_straddlers():
    """uint8 [4, 1, 200] for mode 'L' and filter 0: runs that end one byte before, at, and one byte after the 64-byte steps of the walk (the type byte is byte 0
    of the segment, so pixel x is byte x + 1), and one that starts on the step's last byte."""
    rows = (np.arange(200)[None, None, :] % 199 + 1).repeat(4, axis=0).astype(np.uint8)
    rows[0, 0, 40:62] = 5                                                         # bytes 41 .. 62
    rows[1, 0, 40:63] = 5                                                         # bytes 41 .. 63: ends with the step
    rows[2, 0, 40:64] = 5                                                         # bytes 41 .. 64: one byte into the next
    rows[3, 0, 62:140] = 5                                                        # bytes 63 .. 140: starts on a step's last byte, spans the next whole
    return torch.from_numpy(rows)
