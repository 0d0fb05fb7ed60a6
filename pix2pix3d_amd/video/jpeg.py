"""True colour needs no palette: baseline JPEG streams made where the frames are, and a decoder's view of them.

``encode_jpeg`` turns uint8 [F, H, W, 3] frames into baseline JPEG streams on their own device (``jpeg_coefficients``: colour transform, chroma
subsampling, an integer 8 x 8 DCT and the quantiser; ``jpeg_scan``: Huffman coding in restart intervals, byte stuffing) and ``save_jpeg`` writes a still.
Every frame is a baseline JFIF of its own, made without a codec library.  csrc/video/p3d_video.h states every step in integers; the formulations here are
those rules operation by operation — the definition — and the kernels' bytes equal them.

What a setting costs is measured where the frames are (``quality.py``): ``jpeg_decode`` / ``jpeg_reconstruct`` show what a viewer of
the JPEGs sees without entropy decoding, and ``jpeg_quality_for`` turns a PSNR, SSIM or MS-SSIM (``multiscale.py``; section 2.1ac) target into a quality (``encode_jpeg`` takes ``psnr=``, ``ssim=`` or
``ms_ssim=`` in place of one)."""
import numpy as np
import torch

from .. import _lib, multiscale
from .. import quality as Q
from ..clips import HEADER, MAX_PIXELS, check, check_frames, clip_args, video_lib

JPEG_RESTART, JPEG_BLOCK_BITS = HEADER.constants['P3D_VIDEO_JPEG_RESTART'], HEADER.constants['P3D_VIDEO_JPEG_BLOCK_BITS']
_SUBSAMPLING = {'4:4:4': 0, '4:2:0': 1}
_BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# Annex K.3: (BITS: the number of codes of every length 1 .. 16, HUFFVAL: the symbols in code order) of DC luma, DC chroma, AC luma, AC chroma.
_AC_LUMA_VALUES = bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a53545556'
    '5758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6'
    'd7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa')
_AC_CHROMA_VALUES = bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a5354'
    '55565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3'
    'd4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')
_ANNEX_K = (((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
            ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
            ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), tuple(_AC_LUMA_VALUES)),
            ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), tuple(_AC_CHROMA_VALUES)))


def jpeg_zigzag():
    """int64 [64]: the natural index 8 v + u of every zigzag position — the diagonals v + u in turn, odd ones downwards (v rising), even ones upwards."""
    return torch.tensor(sorted(range(64), key=lambda n: (n // 8 + n % 8, n // 8 if (n // 8 + n % 8) % 2 else n % 8)), dtype=torch.int64)


def jpeg_dct_table():
    """int64 [8, 8]: T[u][x] = round(8192 a(u) cos((2 x + 1) u pi / 16)), a(0) = sqrt(1 / 8), a(u) = 1 / 2 otherwise — the literals of p3d_video.h."""
    u, x = np.arange(8.0)[:, None], np.arange(8.0)[None, :]
    a = np.where(u == 0, np.sqrt(0.125), 0.5)
    return torch.from_numpy(np.round(8192 * a * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64))


def jpeg_dct(samples):
    """int64 [..., 8, 8] (v, u) of integer level-shifted samples [..., 8, 8] (y, x): 8 x the orthonormal DCT by the header's two integer passes,
    r[y][u] = (sum_x T[u][x] s[y][x] + 128) >> 8, then c8[v][u] = (sum_y T[v][y] r[y][u] + 16384) >> 15, with arithmetic shifts."""
    t = jpeg_dct_table()
    r = (torch.matmul(samples.to(torch.int64), t.T) + 128) >> 8
    return (torch.matmul(t, r) + 16384) >> 15


def _check_quality(quality):
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f'quality must be an integer 1 .. 100, got {quality!r}')
    return int(quality)


def jpeg_tables(quality):
    """(luma, chroma): two uint8 [64] quantisation tables in ZIGZAG order on the host — the Annex K base tables under the IJG scaling, scale = 5000 / quality
    (an integer division) below 50 and 200 - 2 quality from 50, entry = clamp((base scale + 50) / 100, 1, 255).  1 <= ``quality`` <= 100."""
    q = _check_quality(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    zigzag = jpeg_zigzag()
    return tuple(((torch.tensor(base, dtype=torch.int64) * scale + 50) // 100).clamp(1, 255).to(torch.uint8)[zigzag] for base in (_BASE_LUMA, _BASE_CHROMA))


class JpegHuffman:
    """The four Annex K tables, in the order DC luma, DC chroma, AC luma, AC chroma: ``bits`` (four tuples of 16: the number of codes of every length) and
    ``values`` (four tuples: the symbols in code order) as a DHT segment states them, and ``lookup`` uint32 [4, 256] on the host: per table and symbol
    length << 16 | code, 0 for a symbol without a code — what ``p3d_video_jpeg_scan`` reads."""

    def __init__(self):
        self.bits, self.values = tuple(b for b, _ in _ANNEX_K), tuple(v for _, v in _ANNEX_K)
        lookup = np.zeros([4, 256], dtype=np.int64)
        for t, (bits, values) in enumerate(_ANNEX_K):
            code, k = 0, 0
            for length, n in enumerate(bits, start=1):                          # the canonical assignment of Annex C
                for _ in range(n):
                    lookup[t, values[k]] = length << 16 | code
                    code, k = code + 1, k + 1
                code <<= 1
        self.lookup = torch.from_numpy(lookup.astype(np.uint32).view(np.int32)).view(torch.int32)      # (torch has little use for uint32: the same 32 bits)


_huffman = None
_on_device = {}                                      # (what, device) -> the constant tables there: uploaded once


def jpeg_huffman():
    """The ``JpegHuffman`` of this module (made once)."""
    global _huffman
    if _huffman is None:
        _huffman = JpegHuffman()
    return _huffman


def _device_tables(what, device, make):
    key = (what, str(device))
    if key not in _on_device:
        _on_device[key] = tuple(t.to(device) for t in make())
    return _on_device[key]


def _check_subsampling(subsampling):
    if subsampling in (0, 1) and not isinstance(subsampling, bool):
        return int(subsampling)
    if subsampling not in _SUBSAMPLING:
        raise ValueError(f"subsampling must be '4:4:4' or '4:2:0' (0 or 1), got {subsampling!r}")
    return _SUBSAMPLING[subsampling]


def jpeg_layout(h, w, subsampling):
    """(MCUs of a row, MCUs of a frame, blocks of an MCU, restart intervals of a frame) of an ``h`` x ``w`` picture."""
    sub = _check_subsampling(subsampling)
    mcu = 8 << sub
    mcus_x, mcus_y = -(-int(w) // mcu), -(-int(h) // mcu)
    return mcus_x, mcus_x * mcus_y, 6 if sub else 3, -(-(mcus_x * mcus_y) // JPEG_RESTART)


def _jpeg_coefficients_torch(frames, luma_q, chroma_q, sub):
    f, h, w = frames.shape[:3]
    mcu = 8 << sub
    hp, wp = -(-h // mcu) * mcu, -(-w // mcu) * mcu
    rows, cols = torch.arange(hp).clamp(max=h - 1), torch.arange(wp).clamp(max=w - 1)      # the last row and column repeat
    rgb = frames[:, rows][:, :, cols].to(torch.int64)
    r, g, b = rgb.unbind(dim=3)
    planes = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
              ((-11059 * r - 21709 * g + 32768 * b + 32768 + (128 << 16)) >> 16).clamp(0, 255),
              ((32768 * r - 27439 * g - 5329 * b + 32768 + (128 << 16)) >> 16).clamp(0, 255)]
    if sub:
        planes[1:] = [(p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2] + 2) >> 2 for p in planes[1:]]
    zigzag = jpeg_zigzag()

    def blocks(plane, q):
        """[F, rows of blocks, columns of blocks, 64]: the quantised coefficients of every 8 x 8 block in zigzag order."""
        hb, wb = plane.shape[1] // 8, plane.shape[2] // 8
        c8 = jpeg_dct(plane.reshape(f, hb, 8, wb, 8).permute(0, 1, 3, 2, 4) - 128).reshape(f, hb, wb, 64)[..., zigzag]
        q = q.to(torch.int64).clamp(min=1)
        return torch.sign(c8) * ((c8.abs() + 4 * q) // (8 * q))
    y, cb, cr = blocks(planes[0], luma_q), blocks(planes[1], chroma_q), blocks(planes[2], chroma_q)
    my, mx = hp // mcu, wp // mcu
    if sub:                                                                       # Y00 Y01 Y10 Y11 of every MCU
        y = y.reshape(f, my, 2, mx, 2, 64).permute(0, 1, 3, 2, 4, 5).reshape(f, my, mx, 4, 64)
    else:
        y = y[:, :, :, None]
    return torch.cat([y, cb[:, :, :, None], cr[:, :, :, None]], dim=3).reshape(f, my * mx, -1, 64).to(torch.int16)


def jpeg_coefficients(frames, tables, subsampling='4:2:0'):
    """int16 [F, n_mcu, 3 or 6, 64]: the quantised DCT coefficients of the frames, MCUs in raster order, the blocks of an MCU Y Cb Cr (4:4:4, an MCU of
    8 x 8 pixels) or Y00 Y01 Y10 Y11 Cb Cr (4:2:0, 16 x 16), every block in zigzag order.  ``tables``: (luma, chroma) uint8 [64] in zigzag order
    (``jpeg_tables``).  The rules — the fixed-point JFIF colour transform, edge replication up to the MCU, the rounded 2 x 2 chroma mean, the two integer DCT
    passes, the rounding quantiser — are p3d_video.h's.  Device tensors: ONE ``p3d_video_jpeg_blocks`` launch; CPU tensors: the torch formulation."""
    f, h, w = check_frames(frames)
    sub = _check_subsampling(subsampling)
    luma_q, chroma_q = (torch.as_tensor(t) for t in tables)
    for t in (luma_q, chroma_q):
        if t.dtype != torch.uint8 or tuple(t.shape) != (64,):
            raise ValueError('jpeg_coefficients: tables must be two uint8 [64] tensors')
    _, n_mcu, bpm, _ = jpeg_layout(h, w, sub)
    if f * h * w == 0:
        return torch.zeros([f, 0, bpm, 64], dtype=torch.int16, device=frames.device)      # no pixel, no MCU
    if not frames.is_cuda:
        return _jpeg_coefficients_torch(frames, luma_q.cpu(), chroma_q.cpu(), sub)
    luma_q, chroma_q = luma_q.to(frames.device).contiguous(), chroma_q.to(frames.device).contiguous()
    out = torch.empty([f, n_mcu, bpm, 64], dtype=torch.int16, device=frames.device)
    with _lib.kernel_timer('video_jpeg_blocks', out):
        code = video_lib().p3d_video_jpeg_blocks(*clip_args(frames), sub, _lib.ptr(luma_q), _lib.ptr(chroma_q), _lib.ptr(out), _lib.stream_of(out))
    check(code, 'video_jpeg_blocks')
    return out


def _bit_length(v):
    """The size category of every entry: the number of bits of its magnitude (0 for 0; the entries stay below 2^11)."""
    a = np.abs(v)
    return sum(((a >> b) > 0).astype(np.int64) for b in range(11))


def _jpeg_scan_numpy(blocks, bpm):
    """The scan bytes of ONE frame: ``blocks`` int64 [n_mcu * bpm, 64].  Every (block, coefficient) slot and every block's end becomes a token of up to 59 bits
    (the ZRLs before a value, its code, its extra bits); the tokens' bit positions are a cumulative sum that restarts, byte-aligned, at every interval."""
    table = jpeg_huffman().lookup.numpy().view(np.uint32).astype(np.int64)
    code, length = table & 0xFFFF, table >> 16
    nb = blocks.shape[0]
    k = np.arange(nb) % bpm
    interval = np.arange(nb) // bpm // JPEG_RESTART
    n_intervals = int(interval[-1]) + 1
    component = k if bpm == 3 else np.maximum(k - 3, 0)
    chroma = (component > 0).astype(np.int64)
    dc, ac = np.clip(blocks[:, 0], -1024, 1023), np.clip(blocks[:, 1:], -1023, 1023)
    pred = np.zeros(nb, dtype=np.int64)
    for c in range(3):                                                            # the previous block of the same component, if the interval holds it
        idx = np.flatnonzero(component == c)
        pred[idx[1:]] = np.where(interval[idx[1:]] == interval[idx[:-1]], dc[idx[:-1]], 0)
    values, lengths = np.zeros([nb, 65], dtype=np.int64), np.zeros([nb, 65], dtype=np.int64)

    def extra(v, size):
        return np.where(v < 0, v - 1, v) & ((1 << size) - 1)
    d = dc - pred
    size = _bit_length(d)
    values[:, 0], lengths[:, 0] = code[chroma, size] << size | extra(d, size), length[chroma, size] + size
    position = np.arange(1, 64)[None, :]
    nonzero = ac != 0
    before = np.maximum.accumulate(np.where(nonzero, position, 0), axis=1)        # the last non-zero position up to here ...
    before = np.concatenate([np.zeros([nb, 1], dtype=np.int64), before[:, :-1]], axis=1)      # ... and before here (0: the DC)
    run = position - before - 1
    size = _bit_length(ac)
    tab = (2 + chroma)[:, None]
    v, n = code[tab, (run & 15) << 4 | size] << size | extra(ac, size), length[tab, (run & 15) << 4 | size] + size
    for j in range(3):                                                            # one ZRL per 16 zeros of the run, in front
        more = (run >> 4) > j
        v, n = np.where(more, code[tab, 0xF0] << n | v, v), np.where(more, n + length[tab, 0xF0], n)
    values[:, 1:64], lengths[:, 1:64] = np.where(nonzero, v, 0), np.where(nonzero, n, 0)
    values[:, 64], lengths[:, 64] = code[2 + chroma, 0], np.where(ac[:, 62] == 0, length[2 + chroma, 0], 0)      # EOB unless coefficient 63 is non-zero

    values, lengths, token_interval = values.reshape(-1), lengths.reshape(-1), np.repeat(interval, 65)
    first = np.cumsum(lengths) - lengths
    interval_bits = np.bincount(token_interval, weights=lengths, minlength=n_intervals).astype(np.int64)
    interval_bytes = (interval_bits + 7) // 8
    base = np.cumsum(interval_bytes) - interval_bytes                              # of an interval, in the unstuffed bytes
    first = first - (np.cumsum(interval_bits) - interval_bits)[token_interval] + 8 * base[token_interval]
    bits = np.zeros(8 * int(interval_bytes.sum()), dtype=np.uint8)
    for b in range(int(lengths.max())):
        on = lengths > b
        bits[first[on] + b] = (values[on] >> (lengths[on] - 1 - b)) & 1
    for b in range(7):                                                            # 1-bits up to the byte
        on = interval_bits + b < 8 * interval_bytes
        bits[8 * base[on] + interval_bits[on] + b] = 1
    raw = np.packbits(bits)
    ff = (raw == 255).astype(np.int64)
    stuffed_before = np.cumsum(ff) - ff
    place = np.arange(raw.shape[0]) + stuffed_before + 2 * np.repeat(np.arange(n_intervals), interval_bytes)
    out = np.zeros(raw.shape[0] + int(ff.sum()) + 2 * (n_intervals - 1), dtype=np.uint8)
    out[place] = raw
    marked = np.arange(n_intervals - 1)                                           # every interval but the last: RSTm after it
    at = base[1:] + np.cumsum(ff)[base[1:] - 1] + 2 * marked
    out[at], out[at + 1] = 255, 0xD0 + (marked & 7)
    return out


def jpeg_scan(coefficients, h, w, subsampling='4:2:0'):
    """``(data uint8 [total], offsets int64 [F + 1])``: the entropy-coded scans of ``coefficients`` (``jpeg_coefficients``' layout, for pictures of ``h`` x ``w``),
    frame i at ``data[offsets[i]:offsets[i + 1]]``; ``data`` on the coefficients' device, ``offsets`` on the host.  A frame is cut into restart intervals of
    ``JPEG_RESTART`` MCUs: each starts byte-aligned with the DC predictors 0, is padded with 1-bits, byte-stuffed and — but for the last — followed by RSTm,
    m = interval index mod 8, so that no interval shares a bit with another.  The Annex K tables (``jpeg_huffman``).  Device tensors: two
    ``p3d_video_jpeg_scan`` launches — the byte length of every interval, then, after their prefix sum, the bytes — with the copy of the lengths to the
    host between them, the ONLY synchronisation (it sizes ``data``).  CPU tensors: the numpy formulation, frame by frame."""
    sub = _check_subsampling(subsampling)
    _, n_mcu, bpm, n_intervals = jpeg_layout(h, w, sub)
    if not torch.is_tensor(coefficients) or coefficients.dtype != torch.int16 or coefficients.ndim != 4:
        raise ValueError('jpeg_scan: coefficients must be an int16 [F, n_mcu, blocks, 64] tensor')
    f = coefficients.shape[0]
    if int(h) < 0 or int(w) < 0 or f * int(h) * int(w) >= MAX_PIXELS:
        raise ValueError(f'jpeg_scan: {f} x {h} x {w} pixels are negative or reach 2^31')
    if f * int(h) * int(w) == 0:
        return torch.zeros([0], dtype=torch.uint8, device=coefficients.device), torch.zeros([f + 1], dtype=torch.int64)
    if tuple(coefficients.shape[1:]) != (n_mcu, bpm, 64):
        raise ValueError(f'jpeg_scan: {h} x {w} at subsampling {subsampling!r} has [{n_mcu}, {bpm}, 64] coefficients a frame, got {list(coefficients.shape[1:])}')
    if not coefficients.is_cuda:
        scans = [_jpeg_scan_numpy(c.reshape(-1, 64).to(torch.int64).numpy(), bpm) for c in coefficients]
        sizes = torch.tensor([0] + [s.shape[0] for s in scans], dtype=torch.int64)
        return torch.from_numpy(np.concatenate(scans)), torch.cumsum(sizes, 0)
    coefficients = coefficients.contiguous()
    huffman, = _device_tables('huffman', coefficients.device, lambda: (jpeg_huffman().lookup,))
    lengths = torch.empty([f, n_intervals], dtype=torch.int32, device=coefficients.device)
    stream = lambda: _lib.stream_of(coefficients)
    with _lib.kernel_timer('video_jpeg_scan_lengths', lengths):
        code = video_lib().p3d_video_jpeg_scan(_lib.ptr(coefficients), f, int(h), int(w), sub, _lib.ptr(huffman), _lib.ptr(lengths), None, None, 0, stream())
    check(code, 'video_jpeg_scan')
    ends = torch.cumsum(lengths.reshape(-1), 0, dtype=torch.int64)
    starts = ends - lengths.reshape(-1)                                            # on the device: the second launch does not wait for the host
    offsets = torch.cat([torch.zeros([1], dtype=torch.int64), torch.cumsum(lengths.cpu().sum(dim=1, dtype=torch.int64), 0)])
    data = torch.empty([int(offsets[-1])], dtype=torch.uint8, device=coefficients.device)
    with _lib.kernel_timer('video_jpeg_scan_bytes', data):
        code = video_lib().p3d_video_jpeg_scan(_lib.ptr(coefficients), f, int(h), int(w), sub, _lib.ptr(huffman), None, _lib.ptr(starts), _lib.ptr(data),
                                               data.shape[0], stream())
    check(code, 'video_jpeg_scan')
    return data, offsets


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + payload


def jpeg_header(h, w, tables, subsampling='4:2:0'):
    """Everything of a baseline JFIF before its scan: SOI, APP0 (JFIF 1.01, square pixels), two DQT, SOF0 (8 bits, three components, Y sampled 2 x 2 at 4:2:0),
    the four Annex K DHT, DRI (``JPEG_RESTART`` MCUs) and SOS.  The scan and EOI (0xFF 0xD9) follow."""
    sub = _check_subsampling(subsampling)
    if not (1 <= int(h) <= 65535 and 1 <= int(w) <= 65535):
        raise ValueError(f'a JPEG is 1 .. 65535 pixels a side, got {h} x {w}')
    huffman = jpeg_huffman()
    out = b'\xff\xd8' + _segment(0xE0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, table in enumerate(tables):
        out += _segment(0xDB, bytes([i]) + bytes(torch.as_tensor(table).cpu().tolist()))
    out += _segment(0xC0, bytes([8]) + int(h).to_bytes(2, 'big') + int(w).to_bytes(2, 'big') + bytes([3, 1, 0x22 if sub else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for i, (bits, values) in enumerate(zip(huffman.bits, huffman.values)):       # Tc << 4 | Th: DC 0, DC 1, AC 0, AC 1
        out += _segment(0xC4, bytes([(i >> 1) << 4 | (i & 1)]) + bytes(bits) + bytes(values))
    out += _segment(0xDD, JPEG_RESTART.to_bytes(2, 'big'))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode_jpeg(frames, quality=90, subsampling='4:2:0', psnr=None, ssim=None, ms_ssim=None):
    """A list of ``bytes``, one complete baseline JFIF per frame of uint8 [F, H, W, 3] (the module's frame contract; on the device or the host, or a numpy
    array): ``jpeg_header``, the frame's scan, EOI.  ``quality`` 1 .. 100 picks the tables (``jpeg_tables``).  From device frames: the two kernels' three
    launches, ONE synchronisation with the host (the interval lengths) and ONE device -> host copy (the scans, a few percent of the frames' bytes).
    ``psnr``, ``ssim`` or ``ms_ssim`` (ONE of them): a target instead of a setting — ``jpeg_quality_for`` picks the quality, ``quality`` plays no part, and
    the tables in the streams (``jpeg_tables`` of the choice) say what it was."""
    frames = torch.as_tensor(frames)
    f, h, w = check_frames(frames)
    if psnr is not None or ssim is not None or ms_ssim is not None:
        _check_target(psnr, ssim, 'encode_jpeg', ms_ssim)
        if f * h * w:
            quality = jpeg_quality_for(frames, psnr, ssim, subsampling, ms_ssim=ms_ssim)[0]
    sub, tables = _check_subsampling(subsampling), jpeg_tables(quality)
    if f == 0:
        return []
    header = jpeg_header(h, w, tables, sub)
    on_device = _device_tables(('quantisation', _check_quality(quality)), frames.device, lambda: tables) if frames.is_cuda else tables
    data, offsets = jpeg_scan(jpeg_coefficients(frames, on_device, sub), h, w, sub)
    data, offsets = data.cpu().numpy().tobytes(), offsets.tolist()
    return [header + data[offsets[i]:offsets[i + 1]] + b'\xff\xd9' for i in range(f)]


def save_jpeg(path, frame, quality=90, subsampling='4:2:0'):
    """One uint8 [H, W, 3] frame, on the device or the host, as a baseline JPEG file (``encode_jpeg``).  Returns its bytes."""
    frame = torch.as_tensor(frame)
    if frame.ndim != 3:
        raise ValueError(f'save_jpeg: frame must be uint8 [H, W, 3], got {tuple(frame.shape)}')
    stream, = encode_jpeg(frame[None], quality, subsampling)
    with open(path, 'wb') as fh:
        fh.write(stream)
    return stream


# ---- the way back: what a setting costs ------------------------------------------------------------------------------------------------------
# A decoder's view of the coefficients without entropy decoding, so that ``quality.compare`` can judge a setting where the frames are, and the search
# that turns a target into a setting.
def jpeg_idct(coefficients):
    """int64 [..., 8, 8] (y, x) of dequantised coefficients [..., 8, 8] (v, u) in natural order: the header's two integer passes, the column pass
    m[y][u] = (sum_v T[v][y] c[v][u] + 512) >> 10, then the row pass s[y][x] = (sum_u T[u][x] m[y][u] + 32768) >> 16 — the level-shifted sample."""
    t = jpeg_dct_table()
    m = (torch.matmul(t.T, coefficients.to(torch.int64)) + 512) >> 10
    return (torch.matmul(m, t) + 32768) >> 16


def jpeg_dequantize(coefficients, tables, subsampling):
    """int64 [F, n_mcu, blocks, 8, 8] (v, u): ``jpeg_coefficients``' int16 blocks times their table's entries (a 0 counts as 1), clamped to int16's range and
    taken out of zigzag order."""
    sub = _check_subsampling(subsampling)
    luma_q, chroma_q = (torch.as_tensor(t).cpu().to(torch.int64).clamp(min=1) for t in tables)
    n_luma = 4 if sub else 1
    q = torch.stack([luma_q] * n_luma + [chroma_q] * 2)                            # [blocks, 64]
    c = (coefficients.to(torch.int64) * q).clamp(-32768, 32767)
    natural = torch.empty_like(c)
    natural[..., jpeg_zigzag()] = c
    return natural.reshape(*c.shape[:-1], 8, 8)


def _jpeg_decode_torch(coefficients, tables, h, w, sub, out):
    f = coefficients.shape[0]
    mcu = 8 << sub
    my, mx = -(-h // mcu), -(-w // mcu)
    s = (jpeg_idct(jpeg_dequantize(coefficients, tables, sub)) + 128).clamp(0, 255).reshape(f, my, mx, -1, 8, 8)

    def plane(blocks):                                                            # [F, my, mx, 8, 8] -> [F, 8 my, 8 mx]
        return blocks.permute(0, 1, 3, 2, 4).reshape(f, my * 8, mx * 8)
    if sub:
        y = s[:, :, :, :4].reshape(f, my, mx, 2, 2, 8, 8).permute(0, 1, 3, 5, 2, 4, 6).reshape(f, my * 16, mx * 16)
        ch, cw = (h + 1) // 2, (w + 1) // 2
        rows, cols = torch.arange(h), torch.arange(w)
        near, cx = rows >> 1, cols >> 1
        far = (near + torch.where(rows & 1 == 1, 1, -1)).clamp(0, ch - 1)
        ox = (cx + torch.where(cols & 1 == 1, 1, -1)).clamp(0, cw - 1)
        bias = torch.where(cols & 1 == 1, 7, 8)
        chroma = []
        for k in (4, 5):
            p = plane(s[:, :, :, k])[:, :ch, :cw]
            v = 3 * p[:, near] + p[:, far]                                        # [F, h, cw]
            chroma.append((3 * v[:, :, cx] + v[:, :, ox] + bias) >> 4)
        cb, cr = chroma
    else:
        y, cb, cr = (plane(s[:, :, :, k]) for k in range(3))
    y, cb, cr = y[:, :h, :w], cb[:, :h, :w] - 128, cr[:, :h, :w] - 128
    rgb = torch.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], dim=3)
    out.copy_(rgb.clamp(0, 255).to(torch.uint8))
    return out


def jpeg_decode(coefficients, tables, h, w, subsampling='4:2:0', out=None):
    """uint8 [F, h, w, 3]: what a decoder shows for ``coefficients`` (``jpeg_coefficients``' layout, for pictures of ``h`` x ``w``) under ``tables`` — no
    entropy decoding, so a quality setting is judged where the frames are.  p3d_video.h states the rules: dequantise and clamp to int16, the inverse of
    the integer DCT in two passes with 26 bits of rounding shifts, + 128 and clamp; at 4:2:0 the triangle filter on the chroma planes (3 : 1 vertically,
    then 3 : 1 horizontally with the roundings 8 and 7, edges replicated); the fixed-point JFIF inverse colour transform; the crop.  Not bit-equal with any
    libjpeg (their inverse DCTs differ by a level here and there), but the same picture.  ``out``: the caller's uint8 [F, h, w, 3] view with contiguous
    pixels and any pitches.  Device tensors: TWO launches of ``p3d_video_jpeg_decode`` (blocks into planes in a scratch buffer, then pixels), no
    synchronisation; CPU tensors: the torch formulation."""
    sub = _check_subsampling(subsampling)
    h, w = int(h), int(w)
    _, n_mcu, bpm, _ = jpeg_layout(h, w, sub)
    if not torch.is_tensor(coefficients) or coefficients.dtype != torch.int16 or coefficients.ndim != 4:
        raise ValueError('jpeg_decode: coefficients must be an int16 [F, n_mcu, blocks, 64] tensor')
    f = coefficients.shape[0]
    if h < 0 or w < 0 or f * h * w >= MAX_PIXELS:
        raise ValueError(f'jpeg_decode: {f} x {h} x {w} pixels are negative or reach 2^31')
    luma_q, chroma_q = (torch.as_tensor(t) for t in tables)
    for t in (luma_q, chroma_q):
        if t.dtype != torch.uint8 or tuple(t.shape) != (64,):
            raise ValueError('jpeg_decode: tables must be two uint8 [64] tensors')
    if out is None:
        out = torch.empty([f, h, w, 3], dtype=torch.uint8, device=coefficients.device)
    elif not torch.is_tensor(out) or tuple(out.shape) != (f, h, w, 3) or out.device != coefficients.device:
        raise ValueError(f'jpeg_decode: out must be uint8 [{f}, {h}, {w}, 3] on {coefficients.device}')
    else:
        check_frames(out, 'jpeg_decode: out')
        if f > 1 and h * w and out.stride(0) < h * out.stride(1):
            raise ValueError(f'jpeg_decode: the frames of out overlap (strides {tuple(out.stride())})')
    if f * h * w == 0:
        return out
    if tuple(coefficients.shape[1:]) != (n_mcu, bpm, 64):
        raise ValueError(f'jpeg_decode: {h} x {w} at subsampling {subsampling!r} has [{n_mcu}, {bpm}, 64] coefficients a frame, got {list(coefficients.shape[1:])}')
    if not coefficients.is_cuda:
        return _jpeg_decode_torch(coefficients, (luma_q, chroma_q), h, w, sub, out)
    coefficients = coefficients.contiguous()
    luma_q, chroma_q = luma_q.to(coefficients.device).contiguous(), chroma_q.to(coefficients.device).contiguous()
    mcu = 8 << sub
    plane = (-(-h // mcu) * mcu) * (-(-w // mcu) * mcu)
    scratch = torch.empty([f * (plane + 2 * (plane >> (2 * sub)))], dtype=torch.uint8, device=coefficients.device)
    with _lib.kernel_timer('video_jpeg_decode', out):
        code = video_lib().p3d_video_jpeg_decode(_lib.ptr(coefficients), f, h, w, sub, _lib.ptr(luma_q), _lib.ptr(chroma_q), _lib.ptr(scratch), scratch.shape[0],
                                                 _lib.ptr(out), out.stride(0), out.stride(1), _lib.stream_of(out))
    check(code, 'video_jpeg_decode')
    return out


def jpeg_reconstruct(frames, quality=90, subsampling='4:2:0'):
    """uint8 [F, H, W, 3] on the frames' device: what a viewer of ``encode_jpeg(frames, quality, subsampling)`` sees — ``jpeg_decode`` of ``jpeg_coefficients``,
    three launches and no synchronisation from device frames."""
    frames = torch.as_tensor(frames)
    f, h, w = check_frames(frames)
    sub, tables = _check_subsampling(subsampling), jpeg_tables(quality)
    if frames.is_cuda:
        tables = _device_tables(('quantisation', _check_quality(quality)), frames.device, lambda: tables)
    return jpeg_decode(jpeg_coefficients(frames, tables, sub), tables, h, w, sub)


def _check_target(psnr, ssim, what, ms_ssim=None):
    """('psnr', 'ssim' or 'ms_ssim', the target): exactly ONE of the three is given.  Two would need a rule for a quality that meets one and not the other; a
    caller who wants several takes the largest of their searches."""
    given = [(k, v) for k, v in (('psnr', psnr), ('ssim', ssim), ('ms_ssim', ms_ssim)) if v is not None]
    if len(given) != 1:
        raise ValueError(f'{what}: give psnr (dB), ssim (0 .. 1) or ms_ssim (0 .. 1), one of them, got psnr={psnr!r}, ssim={ssim!r}, ms_ssim={ms_ssim!r}')
    key, target = given[0]
    if isinstance(target, bool) or not isinstance(target, (int, float)) or target != target or (key != 'psnr' and not 0 <= target <= 1) or (key == 'psnr' and target < 0):
        raise ValueError(f'{what}: {key} must be a number{" 0 .. 1" if key != "psnr" else " >= 0 (dB)"}, got {target!r}')
    return key, float(target)


def jpeg_quality_for(frames, psnr=None, ssim=None, subsampling='4:2:0', sample=8, ms_ssim=None):
    """``(quality, metrics, met)``: the JPEG quality that meets a target — ``psnr`` in dB, ``ssim`` or ``ms_ssim`` in 0 .. 1, ONE of them (``_check_target``)
    — as ``quality.compare`` (for ``ms_ssim``: ``multiscale.ms_ssim`` at five levels, whose dict ``metrics`` then is; both sides at least 176 pixels)
    measures ``jpeg_reconstruct`` against the frames, on at most ``sample`` evenly spaced frames of the clip (the first and the last among them).  A
    bisection of 1 .. 100 in at most seven steps, each three launches for the reconstruction, two for the sums (five for ``ms_ssim``) and ONE host read.
    The measure need not rise with the quality, so the promise is a post-condition, ``mesh.simplify_to``'s: the quality returned met the target as measured
    (``metrics`` is its ``compare`` dict), and the quality below it was tried and did not (unless it is 1); if 100 does not meet it,
    ``(100, its metrics, False)``.  A clip without a sample — or, for ``ssim``, without a window — measures NaN, which meets nothing; for ``ms_ssim`` a
    clip under 176 pixels a side is a ValueError."""
    frames = torch.as_tensor(frames)
    f, h, w = check_frames(frames)
    key, target = _check_target(psnr, ssim, 'jpeg_quality_for', ms_ssim)
    sub = _check_subsampling(subsampling)
    if key == 'ms_ssim':
        measure = multiscale.ms_ssim
    else:
        measure = Q.compare
    if isinstance(sample, bool) or int(sample) != sample or int(sample) < 1:
        raise ValueError(f'jpeg_quality_for: sample must be an integer >= 1, got {sample!r}')
    n = int(sample)
    if f > n:
        frames = frames[[0] if n == 1 else [(i * (f - 1)) // (n - 1) for i in range(n)]]
    measured = {}
    low, high = 1, 101                                                            # the answer lies in low .. high; 101: none
    while low < high:
        mid = (low + high) // 2
        measured[mid] = measure(jpeg_reconstruct(frames, mid, sub), frames)
        if measured[mid][key] >= target:
            high = mid
        else:
            low = mid + 1
    return (low, measured[low], True) if low <= 100 else (100, measured[100], False)
