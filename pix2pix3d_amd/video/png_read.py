"""The way back from a lossless file: PNG and APNG read where the frames are judged.

``png_parse`` reads a file's chunks on the host (``png.png_chunks``) — a few hundred bytes beside the data.  ``png_inflate`` is RFC 1951 inflate:
``p3d_video_png_inflate``, a lane per PART, a run of whole deflate blocks that begins on a byte, with a status per part for bytes that did not come from
us.  ``png_unfilter`` is the inverse of ``png.png_filter``: ``p3d_video_png_unfilter``, a skewed wavefront over the rows.  Both are integer functions of
the bytes: csrc/video/p3d_video.h states them, the Python / numpy formulations here are the definition, the device results equal them.  ``decode_png``
puts the three together, ``load_png`` / ``decode_apng`` / ``check_png`` / ``png_rgb`` stand on it.  Our own files (all six modes of ``encode_png``; with
``index=True`` a part a segment) and anybody's 8-bit and 16-bit-grey files are served; Adam7, depths 1, 2 and 4 and 16-bit colour are refused by name."""
import collections
import fractions

import numpy as np
import torch

from ..clips import HEADER, MAX_PIXELS
from .jpeg_read import _upload
from .png import (_ADLER, _CL_ORDER, _LENGTH_BASE, _LENGTH_EXTRA, PNG_MODES, _check_filtered, _inflate_launch, _unfilter_launch, png_chunks, png_counts,
                  png_segment_rows)

PNG_STATUS = {name: HEADER.constants['P3D_VIDEO_PNG_STATUS_' + name] for name in
              ('BLOCK_TYPE', 'STORED', 'CODE_LENGTHS', 'NO_CODE', 'DISTANCE', 'OVERFLOW', 'EXHAUSTED', 'LEFTOVER', 'BOUNDARY', 'SHORT', 'FILTER', 'ADLER')}
PNG_INFLATE_LANES = HEADER.constants['P3D_VIDEO_PNG_INFLATE_LANES']
_S = PNG_STATUS
_DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
_DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)      # RFC 1951 section 3.2.5
_MODE_OF = {(colour_type, depth): mode for mode, (_, colour_type, depth) in PNG_MODES.items()}
_COLOUR_TYPES = {0: 'grey', 2: 'RGB', 3: 'palette', 4: 'grey + alpha', 6: 'RGBA'}
PngInfo = collections.namedtuple('PngInfo', 'h w mode depth colour_type palette transparency streams delays n_plays index')
PngInfo.__doc__ = """What ``png_parse`` reads from a PNG or APNG: ``h``, ``w``; ``mode``, a ``PNG_MODES`` key, with ``depth`` and ``colour_type`` as IHDR has them;
``palette`` uint8 [n, 3] or None; ``transparency`` the raw tRNS payload or None (returned, not applied); ``streams`` the zlib stream of every frame, its
IDAT / fdAT chunks joined; ``delays`` per frame a ``fractions.Fraction`` of a second, None for a still; ``n_plays`` acTL's (0: for ever), None for a
still; ``index`` per frame None or ``(segment_rows, (offset of every segment but the first in the frame's zlib stream))`` from a seGM chunk."""


def png_status_names(bits):
    """The names of the ``PNG_STATUS`` bits set in ``bits``."""
    return [name for name, bit in PNG_STATUS.items() if int(bits) & bit]


# ---- the file -------------------------------------------------------------------------------------------------------------------------------------
def _check_zlib(stream, frame):
    if len(stream) < 6:
        raise ValueError(f'png_parse: the zlib stream of frame {frame} has {len(stream)} bytes: shorter than 6 (header, one block, Adler-32)')
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8 or cmf >> 4 > 7:
        raise ValueError(f'png_parse: the zlib header of frame {frame} is not deflate with a window of at most 32 K (CMF 0x{cmf:02X})')
    if flg & 0x20:
        raise ValueError(f'png_parse: the zlib header of frame {frame} asks for a preset dictionary')
    if (cmf << 8 | flg) % 31:
        raise ValueError(f'png_parse: the zlib header of frame {frame} fails FCHECK')


def png_parse(data):
    """The ``PngInfo`` of one PNG or APNG given as ``bytes``: everything ``decode_png`` needs.  ValueError, naming the reason, for what the reader does not
    serve — Adam7 interlacing, bit depths 1, 2 and 4, 16-bit samples other than grey, an unknown colour type, compression or filter method — and for a file
    that is not whole: a bad signature or CRC (``png_chunks``), IHDR of the wrong length, no PLTE before the IDAT of a palette file or one after it, no
    IDAT, IDAT chunks apart, a zlib header that is not deflate with a window of at most 32 K and no preset dictionary or that fails FCHECK, a stream
    shorter than 6 bytes; for an APNG also an fcTL that is not the whole canvas at offset 0, a dispose other than none (0) or a blend other than source
    (0), sequence numbers out of order, a frame count other than acTL's, a default image outside the animation; and a seGM whose count of segments does
    not fit the height."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise ValueError(f'png_parse: data must be bytes, got {type(data).__name__}')
    chunks = png_chunks(bytes(data))
    ihdr = chunks[0][1]
    if len(ihdr) != 13:
        raise ValueError(f'png_parse: IHDR has {len(ihdr)} bytes, not 13')
    w, h = int.from_bytes(ihdr[0:4], 'big'), int.from_bytes(ihdr[4:8], 'big')
    depth, colour_type, compression, filter_method, interlace = ihdr[8:13]
    if not (1 <= w < 1 << 31 and 1 <= h < 1 << 31):
        raise ValueError(f'png_parse: a PNG is 1 .. 2^31 - 1 pixels a side, got {h} x {w}')
    if colour_type not in _COLOUR_TYPES or depth not in (1, 2, 4, 8, 16):
        raise ValueError(f'png_parse: colour type {colour_type} at depth {depth} is no PNG')
    if compression or filter_method:
        raise ValueError(f'png_parse: compression method {compression} / filter method {filter_method}: only 0 / 0 is PNG')
    if interlace:
        raise ValueError('png_parse: Adam7 interlacing is not served')
    if depth < 8:
        raise ValueError(f'png_parse: bit depth {depth} is not served: 8, and 16 for grey, are')
    if (colour_type, depth) not in _MODE_OF:
        raise ValueError(f'png_parse: 16-bit samples other than grey ({_COLOUR_TYPES[colour_type]}) are not served')
    mode = _MODE_OF[colour_type, depth]
    palette = transparency = actl = None
    streams, delays, index, pending, sequence, previous = [], [], [], None, 0, None

    def next_sequence(payload, kind):
        nonlocal sequence
        if len(payload) < 4 or int.from_bytes(payload[:4], 'big') != sequence:
            raise ValueError(f'png_parse: APNG sequence numbers out of order: {kind} carries {int.from_bytes(payload[:4], "big")}, {sequence} is due')
        sequence += 1
    for kind, payload in chunks[1:-1]:
        if kind == b'IHDR':
            raise ValueError('png_parse: a second IHDR')
        if kind == b'PLTE':
            if streams:
                raise ValueError('png_parse: PLTE after IDAT')
            if len(payload) % 3 or not 3 <= len(payload) <= 768:
                raise ValueError(f'png_parse: PLTE has {len(payload)} bytes: 1 .. 256 colours of 3 are a palette')
            palette = torch.tensor(list(payload), dtype=torch.uint8).reshape(-1, 3)
        elif kind == b'tRNS':
            transparency = payload
        elif kind == b'acTL':
            if len(payload) != 8 or streams:
                raise ValueError('png_parse: acTL has the wrong length or comes after IDAT')
            actl = (int.from_bytes(payload[:4], 'big'), int.from_bytes(payload[4:], 'big'))
        elif kind == b'fcTL':
            if len(payload) != 26:
                raise ValueError(f'png_parse: fcTL has {len(payload)} bytes, not 26')
            next_sequence(payload, 'fcTL')
            fw, fh, fx, fy = (int.from_bytes(payload[4 + 4 * i:8 + 4 * i], 'big') for i in range(4))
            if (fw, fh, fx, fy) != (w, h, 0, 0):
                raise ValueError(f'png_parse: fcTL frame {len(delays)} is {fh} x {fw} at ({fx}, {fy}), not the whole canvas at offset 0: sub-rectangles are not served')
            if payload[24] != 0 or payload[25] != 0:
                raise ValueError(f'png_parse: fcTL frame {len(delays)} has dispose {payload[24]} / blend {payload[25]}: only none (0) / source (0) is served')
            num, den = int.from_bytes(payload[20:22], 'big'), int.from_bytes(payload[22:24], 'big')
            delays.append(fractions.Fraction(num, den or 100))
        elif kind == b'seGM':
            if len(payload) < 4 or len(payload) % 4:
                raise ValueError(f'png_parse: seGM has {len(payload)} bytes: uint32 segment_rows and uint32 offsets')
            values = [int.from_bytes(payload[i:i + 4], 'big') for i in range(0, len(payload), 4)]
            if values[0] < 1 or len(values) != -(-h // values[0]):
                raise ValueError(f'png_parse: seGM lists {len(values)} segments of {values[0]} rows, the height {h} makes {-(-h // max(values[0], 1))}')
            pending = (values[0], tuple(values[1:]))
        elif kind == b'IDAT':
            if streams and previous != b'IDAT':
                raise ValueError('png_parse: IDAT chunks apart: another chunk stands between them')
            if colour_type == 3 and palette is None:
                raise ValueError('png_parse: a palette file without PLTE before IDAT')
            if actl is not None and not delays:
                raise ValueError('png_parse: the default image is not part of the animation (no fcTL before IDAT): not served')
            if not streams:
                streams.append([])
                index.append(pending)
                pending = None
            streams[0].append(payload)
        elif kind == b'fdAT':
            next_sequence(payload, 'fdAT')
            if not streams or len(delays) < 2:
                raise ValueError('png_parse: fdAT without an fcTL of its own after IDAT')
            if len(delays) > len(streams):
                streams.append([])
                index.append(pending)
                pending = None
            streams[-1].append(payload[4:])
        previous = kind
    if not streams:
        raise ValueError('png_parse: no IDAT')
    if actl is not None and (len(streams) != actl[0] or len(delays) != actl[0]):
        raise ValueError(f'png_parse: acTL announces {actl[0]} frames, the file holds {len(streams)}')
    if actl is None and (delays or len(streams) > 1):
        raise ValueError('png_parse: fcTL / fdAT without acTL')
    streams = [b''.join(s) for s in streams]
    for i, s in enumerate(streams):
        _check_zlib(s, i)
    return PngInfo(h, w, mode, depth, colour_type, palette, transparency, streams, delays if actl is not None else None, actl[1] if actl is not None else None,
                   index)


# ---- inflate: the definition ------------------------------------------------------------------------------------------------------------------------
class _Bits:
    """The bits of data[begin:end), least significant first; past the end zeros, and reading one sets EXHAUSTED."""

    def __init__(self, data, begin, end):
        self.data, self.at, self.end, self.status = data, 8 * begin, 8 * end, 0

    def peek(self, n):                                                            # the next n <= 32 bits, none of them read yet
        i = self.at >> 3
        return (int.from_bytes(self.data[i:max(min(i + 5, self.end >> 3), i)], 'little') >> (self.at & 7)) & ((1 << n) - 1)

    def take(self, n):
        v = self.peek(n)
        self.at += n
        if n and self.at > self.end:
            self.status |= _S['EXHAUSTED']
        return v


def _code(lengths):
    """{(length, code): symbol} of the canonical code with these lengths (RFC 1951 section 3.2.2), or None for an over-subscribed one."""
    if sum(1 << (15 - l) for l in lengths if l) > 1 << 15:
        return None
    table, code = {}, 0
    for bits in range(1, 16):
        for s, l in enumerate(lengths):
            if l == bits:
                table[bits, code] = s
                code += 1
        code <<= 1
    return table


_FIXED = (_code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _code([5] * 32))


def _symbol(b, table):
    peek, code = b.peek(15), 0
    for length in range(1, 16):
        code = code << 1 | ((peek >> (length - 1)) & 1)
        if (length, code) in table:
            b.take(length)
            return table[length, code]
    b.take(15)
    b.status |= _S['NO_CODE']
    return -1


def _dynamic(b):
    n_lit, n_dist, n_cl = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    if b.status:
        return None
    if n_lit > 286 or n_dist > 30:
        b.status |= _S['CODE_LENGTHS']
        return None
    cl = [0] * 19
    for s in _CL_ORDER[:n_cl]:
        cl[s] = b.take(3)
    if b.status:
        return None
    cl = _code(cl)
    if cl is None:
        b.status |= _S['CODE_LENGTHS']
        return None
    lengths = []
    while len(lengths) < n_lit + n_dist:
        v = _symbol(b, cl)
        if b.status:
            return None
        if v < 16:
            lengths.append(v)
            continue
        if v == 16:
            if not lengths:
                b.status |= _S['CODE_LENGTHS']
                return None
            value, repeat = lengths[-1], 3 + b.take(2)
        else:
            value, repeat = 0, 3 + b.take(3) if v == 17 else 11 + b.take(7)
        if b.status:
            return None
        if len(lengths) + repeat > n_lit + n_dist:
            b.status |= _S['CODE_LENGTHS']
            return None
        lengths += [value] * repeat
    lit, dist = _code(lengths[:n_lit]), _code(lengths[n_lit:])
    if lit is None or dist is None:
        b.status |= _S['CODE_LENGTHS']
        return None
    return lit, dist


def _inflate_part(data, in_begin, in_end, out, out_begin, out_end, final):
    """The rules of p3d_video.h for ONE part, in plain Python: the status; ``out`` (a bytearray of zeros) receives the bytes."""
    b, q = _Bits(data, in_begin, in_end), out_begin
    while True:
        last, kind = b.take(1), b.take(2)
        if b.status:
            return b.status
        if kind == 3:
            return _S['BLOCK_TYPE']
        if last and not final:
            return _S['BOUNDARY']
        if kind == 0:
            b.take(-b.at & 7)
            v = b.take(32)
            if b.status:
                return b.status
            n = v & 0xFFFF
            if n != (~v >> 16) & 0xFFFF:
                return _S['STORED']
            p = b.at >> 3
            have, room = in_end - p, out_end - q
            k = min(n, have, room)
            out[q:q + k] = data[p:p + k]
            b.at, q = b.at + 8 * k, q + k
            if k < n:
                return _S['EXHAUSTED'] if have <= k else _S['OVERFLOW']
        else:
            tables = _FIXED if kind == 1 else _dynamic(b)
            if b.status:
                return b.status
            lit, dist = tables
            while True:
                v = _symbol(b, lit)
                if b.status:
                    return b.status
                if v < 256:
                    if q >= out_end:
                        return _S['OVERFLOW']
                    out[q] = v
                    q += 1
                    continue
                if v == 256:
                    break
                if v >= 286:
                    return _S['NO_CODE']
                length = _LENGTH_BASE[v - 257] + b.take(_LENGTH_EXTRA[v - 257])
                if b.status:
                    return b.status
                d = _symbol(b, dist)
                if b.status:
                    return b.status
                if d >= 30:
                    return _S['NO_CODE']
                distance = _DIST_BASE[d] + b.take(_DIST_EXTRA[d])
                if b.status:
                    return b.status
                if distance > q - out_begin:
                    return _S['DISTANCE']
                for _ in range(length):
                    if q >= out_end:
                        return _S['OVERFLOW']
                    out[q] = out[q - distance]
                    q += 1
        if (last if final else b.at == b.end):
            break
    status = 0
    if final and (b.end - b.at) >> 3 > 0:
        status |= _S['LEFTOVER']
    if q < out_end:
        status |= _S['SHORT']
    return status


def png_inflate(data, parts, out_bytes):
    """``(out uint8 [out_bytes], status int32 [n_parts])``: RFC 1951 inflate of the raw deflate bytes ``data`` uint8 [n] — zlib streams without their two
    header bytes and four Adler bytes — cut into ``parts`` int64 [n_parts, 5]: (in_begin, in_end, out_begin, out_end, final) a row, clamped to the buffers.
    A part is a run of whole deflate blocks that begins on a byte and is decoded on its own into its range of ``out``; a foreign stream is ONE part with
    final = 1, a stream whose segment boundaries are known (``encode_png(index=True)``) a part a segment.  ``status`` is 0 for a part that decoded cleanly
    and filled its range, else the ``PNG_STATUS`` bits that stopped it — what it wrote stays, the rest of its range is zero, no other part is touched.  If
    the parts of a stream tile its bytes and its output and all report 0, ``out`` equals a serial decode; a wrong list of parts shows as a status.
    Device tensors: one asynchronous fill and ONE launch of ``p3d_video_png_inflate``, a lane per part, and no synchronisation.  CPU tensors: the
    definition, plain Python that reads one bit at a time — correct, but slow (a second a megabyte of output, about).  The parallel unit is the part: a
    foreign stream is one lane a frame (DESIGN.md section 2.1z has the figures)."""
    if not torch.is_tensor(data) or data.dtype != torch.uint8 or data.ndim != 1:
        raise ValueError('png_inflate: data must be a uint8 [n] tensor')
    if not torch.is_tensor(parts) or parts.dtype != torch.int64 or parts.ndim != 2 or parts.shape[1] != 5:
        raise ValueError('png_inflate: parts must be an int64 [n_parts, 5] tensor')
    out_bytes = int(out_bytes)
    if not 0 <= out_bytes < MAX_PIXELS or parts.shape[0] >= MAX_PIXELS:
        raise ValueError(f'png_inflate: {out_bytes} output bytes or {parts.shape[0]} parts are negative or reach 2^31')
    device, n_parts = data.device, parts.shape[0]
    if n_parts == 0:
        return torch.zeros([out_bytes], dtype=torch.uint8, device=device), torch.zeros([0], dtype=torch.int32, device=device)
    if not data.is_cuda:
        raw, out, status = bytes(data.contiguous().numpy()), bytearray(out_bytes), []
        for in_begin, in_end, out_begin, out_end, final in parts.cpu().tolist():
            in_begin = min(max(in_begin, 0), len(raw))
            out_begin = min(max(out_begin, 0), out_bytes)
            status.append(_inflate_part(raw, in_begin, min(max(in_end, in_begin), len(raw)), out, out_begin, min(max(out_end, out_begin), out_bytes), final != 0))
        return torch.frombuffer(out, dtype=torch.uint8) if out_bytes else torch.zeros([0], dtype=torch.uint8), torch.tensor(status, dtype=torch.int32)
    data, parts = data.contiguous(), parts.to(device).contiguous()
    out = torch.empty([out_bytes], dtype=torch.uint8, device=device)
    status = torch.empty([n_parts], dtype=torch.int32, device=device)
    _inflate_launch(data, parts, out, status)
    return out, status


# ---- un-filtering -------------------------------------------------------------------------------------------------------------------------------------
def _png_unfilter_numpy(rows, bpp):
    """(uint8 [H, n], the FILTER bit or 0) of ONE frame's filtered rows uint8 [H, 1 + n]: the inverse of ``png._png_filter_numpy``, row after row.  None and
    Up are whole-row sums, Sub a running sum per channel; Average and Paeth chain through the byte just made, so they are a loop."""
    h, n = rows.shape[0], rows.shape[1] - 1
    out, status = np.zeros([h, n], dtype=np.int64), 0
    above = np.zeros(n, dtype=np.int64)
    for y in range(h):
        kind, x = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        if kind > 4:
            kind, status = 0, _S['FILTER']
        if kind == 0:
            cur = x
        elif kind == 2:
            cur = (x + above) & 255
        elif kind == 1:
            pad = (-n) % bpp
            cur = (np.cumsum(np.concatenate([x, np.zeros(pad, dtype=np.int64)]).reshape(-1, bpp), axis=0) & 255).reshape(-1)[:n]
        else:
            r, up, cur = x.tolist(), above.tolist(), [0] * n
            for i in range(n):
                a, b, c = (cur[i - bpp], up[i], up[i - bpp]) if i >= bpp else (0, up[i], 0)
                if kind == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[i] = (r[i] + pred) & 255
            cur = np.array(cur, dtype=np.int64)
        out[y] = above = cur
    return out.astype(np.uint8), status


def png_unfilter(filtered, bpp, out=None):
    """``(frames uint8 [F, H, W] (bpp 1) or [F, H, W, bpp], status int32 [F])``: the exact inverse of ``png_filter`` on ``filtered`` uint8 [F, H, 1 + W bpp],
    every frame on its own, ``bpp`` 1 .. 8 bytes a pixel (6 and 8 are 16-bit colour, which ``png_parse`` refuses and the rule does not).  A row's type
    byte above 4 sets the frame's ``FILTER`` status bit, and the row is taken as type 0.  ``out``: a clip of that shape, contiguous pixels and any pitches
    (a window of a larger canvas), that receives the frames; bytes between its rows stay untouched.  Device tensors: ONE ``p3d_video_png_unfilter``
    launch, no synchronisation; CPU tensors: the numpy formulation."""
    f, h, r = _check_filtered(filtered, 'png_unfilter')
    if isinstance(bpp, bool) or int(bpp) != bpp or not 1 <= int(bpp) <= 8 or (r - 1) % int(bpp) or r < 1:
        raise ValueError(f'png_unfilter: bpp must be 1 .. 8 and divide the {r - 1} bytes of a row, got {bpp!r}')
    bpp = int(bpp)
    w = (r - 1) // bpp
    shape = [f, h, w] if bpp == 1 else [f, h, w, bpp]
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=filtered.device)
    strides = tuple(out.stride()) + (1,) * (4 - out.ndim) if torch.is_tensor(out) else ()
    if (not torch.is_tensor(out) or out.dtype != torch.uint8 or list(out.shape) != shape or out.device != filtered.device or
            (f * h * w and (strides[3] != 1 or strides[2] != bpp or strides[1] < bpp * w or strides[0] < 0))):
        raise ValueError(f'png_unfilter: out must be a uint8 {shape} clip on the device of filtered with contiguous pixels')
    if f * h * w == 0:
        return out, torch.zeros([f], dtype=torch.int32, device=filtered.device)
    filtered = filtered.contiguous()
    if not filtered.is_cuda:
        frames, status = zip(*[_png_unfilter_numpy(x.numpy(), bpp) for x in filtered])
        out.copy_(torch.from_numpy(np.stack(frames)).reshape(shape))
        return out, torch.tensor(status, dtype=torch.int32)
    status = torch.empty([f], dtype=torch.int32, device=filtered.device)
    _unfilter_launch(filtered, bpp, out, status)
    return out, status


# ---- files to frames ----------------------------------------------------------------------------------------------------------------------------------
def _adler_of(filtered, rows):
    """int64 [F]: the Adler-32 of every frame's filtered bytes from ``png_counts``' pairs a segment of ``rows`` rows (one launch), combined in int64 torch
    ops on the frames' device: with a = sum b and c = sum (L - i) b_i of a segment of L bytes, s2 += L s1 + c, then s1 += a, from s1 = 1, s2 = 0."""
    f, h, r = filtered.shape
    rows = min(rows, h)
    stats = png_counts(filtered, rows).to(torch.int64)
    a, c = stats[..., -2], stats[..., -1]
    sizes = (h * r - torch.arange(a.shape[1], device=filtered.device) * (rows * r)).clamp(max=rows * r)
    before = (1 + torch.cumsum(a, dim=1) - a) % _ADLER
    s1 = (1 + a.sum(dim=1)) % _ADLER
    s2 = ((sizes % _ADLER) * before + c).sum(dim=1) % _ADLER
    return s2 << 16 | s1


def _decode(infos, device, errors, verify, index, what):
    if errors not in ('raise', 'status'):
        raise ValueError(f"{what}: errors is 'raise' or 'status', got {errors!r}")
    device = torch.device('cpu' if device is None else device)
    if not infos:
        raise ValueError(f'{what}: no stream')
    h, w, mode = infos[0].h, infos[0].w, infos[0].mode
    for i, info in enumerate(infos):
        if (info.h, info.w, info.mode) != (h, w, mode):
            raise ValueError(f'{what}: stream {i} is {info.h} x {info.w} {info.mode}, stream 0 {h} x {w} {mode}: one call, one size and mode')
    bpp = PNG_MODES[mode][0]
    r = 1 + w * bpp
    streams = [s for info in infos for s in info.streams]
    indices = [ix if index else None for info in infos for ix in info.index]
    f = len(streams)
    if f * h * r >= MAX_PIXELS:
        raise ValueError(f'{what}: {f} x {h} x {w} pixels of {bpp} bytes reach 2^31')
    begins = np.cumsum([0] + [len(s) - 6 for s in streams])
    parts, slot = [], []
    for k, (s, ix) in enumerate(zip(streams, indices)):
        rows, firsts = ix if ix is not None else (h, ())
        cuts = [int(begins[k])] + [int(begins[k]) + o - 2 for o in firsts] + [int(begins[k + 1])]
        for j in range(len(cuts) - 1):
            parts.append((cuts[j], cuts[j + 1], (k * h + j * rows) * r, (k * h + min((j + 1) * rows, h)) * r, int(j == len(cuts) - 2)))
            slot.append((k, j))
    most = max(j for _, j in slot) + 1
    n = len(parts)
    # ONE copy up: the parts, where the status of every part goes, every stream's Adler-32, then the compressed bytes
    words = np.concatenate([np.array(parts, dtype=np.int64).reshape(-1), np.array([k * most + j for k, j in slot], dtype=np.int64),
                            np.array([int.from_bytes(s[-4:], 'big') for s in streams], dtype=np.int64)])
    up = _upload(np.concatenate([words.view(np.uint8), np.frombuffer(b''.join(s[2:-4] for s in streams), dtype=np.uint8)]), device)
    table = up[:8 * words.shape[0]].view(torch.int64)
    filtered, part_status = png_inflate(up[8 * words.shape[0]:], table[:5 * n].view(n, 5), f * h * r)
    filtered = filtered.view(f, h, r)
    frames, frame_status = png_unfilter(filtered, bpp)
    status = torch.zeros([f * most], dtype=torch.int32, device=device)
    status[table[5 * n:6 * n]] = part_status
    status = status.view(f, most)
    if verify:
        wrong = _adler_of(filtered, png_segment_rows(w, bpp)) != table[6 * n:]
        frame_status = frame_status | (wrong.to(torch.int32) * _S['ADLER'])
    status[:, 0] |= frame_status
    if errors == 'status':
        return frames, status
    bad = status.cpu().nonzero()
    if bad.shape[0]:
        i, j = bad[0].tolist()
        hint = ': the index (seGM) does not describe the stream; index=False decodes without it' if indices[i] is not None else ''
        raise ValueError(f'{what}: frame {i}, part {j} does not decode: {", ".join(png_status_names(status[i, j]))}{hint}'
                         f' ({bad.shape[0]} damaged part{"s" if bad.shape[0] > 1 else ""} in all)')
    return frames


def decode_png(streams, device=None, errors='raise', verify=True, index=True):
    """uint8 [F, H, W] or [F, H, W, bpp] on ``device`` (default: the host): the frames of a list of PNG ``bytes`` of ONE size and mode — ours or anybody's that
    ``png_parse`` accepts — in exactly the layout ``encode_png`` takes: 'I;16' is [F, H, W, 2] big-endian byte pairs, 'P' the indices (``png_rgb`` expands
    them); an APNG among them gives all its frames.  The chunks are parsed on the host; everything goes to the device in ONE copy; then one ``png_inflate``
    (a fill and a launch) for all frames and one ``png_unfilter`` launch.  ``verify=True``: one more launch (``png_counts``) and a few int64 torch ops
    compare the Adler-32 of what was inflated with every stream's last four bytes, on the device: the ``ADLER`` bit.  ``index=True`` uses the segment
    index of files written with ``encode_png(index=True)``: a part a segment; ``index=False`` ignores it, every stream is one part — one lane.
    ``errors='raise'``: a part that does not decode cleanly is a ValueError naming frame, part and reason — one small device -> host copy.
    ``errors='status'``: ``(frames, status)`` with status int32 [F, the most parts of a frame] (``PNG_STATUS`` bits, 0: clean or no such part; the frame's
    ``FILTER`` and ``ADLER`` bits in column 0) on the device, and no synchronisation; a damaged part shows what it decoded and zeros after it."""
    return _decode([png_parse(s) for s in streams], device, errors, verify, index, 'decode_png')


def load_png(path, device=None):
    """``(frame, info)``: the first frame of a PNG file, uint8 [H, W] or [H, W, bpp] on ``device`` (``decode_png``), and its ``PngInfo``."""
    with open(path, 'rb') as fh:
        info = png_parse(fh.read())
    return _decode([info._replace(streams=info.streams[:1], index=info.index[:1])], device, 'raise', True, True, 'load_png')[0], info


def decode_apng(path, device=None):
    """``(frames, fps)``: every frame of an APNG (or the one of a PNG) on ``device``, and the frame rate as ``save_apng`` took it — an int where the delay is
    one over a whole number, else a ``fractions.Fraction``; None for a still."""
    with open(path, 'rb') as fh:
        info = png_parse(fh.read())
    fps = None
    if info.delays and info.delays[0] > 0:
        rate = 1 / info.delays[0]
        fps = int(rate) if rate.denominator == 1 else rate
    return _decode([info], device, 'raise', True, True, 'decode_apng'), fps


def check_png(path_or_streams, frames):
    """True where the file (a path) or the list of PNG ``bytes`` holds exactly ``frames`` — ``torch.equal`` on the frames' device, after ``decode_png`` there."""
    if isinstance(path_or_streams, (list, tuple)):
        infos = [png_parse(s) for s in path_or_streams]
    else:
        with open(path_or_streams, 'rb') as fh:
            infos = [png_parse(fh.read())]
    frames = torch.as_tensor(frames)
    shown = _decode(infos, frames.device, 'raise', True, True, 'check_png')
    return shown.shape == frames.shape and torch.equal(shown, frames)


def png_rgb(frames, info):
    """uint8 [..., 3]: ``decode_png``'s frames of the file ``info`` describes as RGB, in torch ops on their device: 'P' through the palette, 'L' three times,
    'LA' and 'RGBA' without their alpha, 'I;16' by its high byte.  tRNS is not applied."""
    mode = info.mode if isinstance(info, PngInfo) else info
    if mode == 'P':
        return info.palette.to(frames.device)[frames.to(torch.int64)]
    if mode == 'RGB':
        return frames
    if mode == 'RGBA':
        return frames[..., :3]
    grey = frames if mode == 'L' else frames[..., 0]
    return grey[..., None].expand(*grey.shape, 3)
