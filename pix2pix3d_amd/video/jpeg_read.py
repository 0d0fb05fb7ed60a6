"""The way back from a file: baseline JPEG entropy decoding, so that clips are read back where they are judged.

``jpeg.jpeg_decode`` starts from coefficients; a file holds their Huffman codes.  ``jpeg_parse`` reads a baseline JPEG's header on the host — a few hundred
bytes — and ``jpeg_unscan`` is the entropy decoder: ``p3d_video_jpeg_unscan``, a lane per restart interval, with a status per interval for bytes that did
not come from us.  It is an integer function of the bytes: csrc/video/p3d_video.h states it, the numpy formulation here is the definition, the device
result equals it.  ``decode_jpeg`` / ``load_jpeg`` put the two in front of ``jpeg_decode``.  Our own streams and libjpeg's (optimised tables, any restart
interval, grey) are served; progressive, 4:2:2 and 12-bit are refused by name."""
import collections

import numpy as np
import torch

from .. import _lib
from ..clips import HEADER, MAX_PIXELS, check, video_lib
from .jpeg import JPEG_RESTART, _ANNEX_K, _check_subsampling, _device_tables, jpeg_decode, jpeg_layout

JPEG_LOOKUP_BITS, JPEG_TABLE_WORDS = HEADER.constants['P3D_VIDEO_JPEG_LOOKUP_BITS'], HEADER.constants['P3D_VIDEO_JPEG_TABLE_WORDS']
JPEG_STATUS = {name: HEADER.constants['P3D_VIDEO_JPEG_STATUS_' + name] for name in ('NO_CODE', 'RUN', 'SIZE', 'EXHAUSTED', 'LEFTOVER')}
JpegInfo = collections.namedtuple('JpegInfo', 'h w subsampling components tables huffman restart scan intervals')
JpegInfo.__doc__ = """What ``jpeg_parse`` reads from a baseline JPEG: ``h``, ``w``; ``subsampling`` '4:4:4' or '4:2:0' and ``components`` 3 — or 1, a grey stream,
laid out as 4:4:4 whose chroma tables equal its luma tables; ``tables`` (luma, chroma) uint8 [64] in zigzag order, as ``jpeg_tables`` returns them;
``huffman`` the (BITS, HUFFVAL) of DC luma, DC chroma, AC luma, AC chroma; ``restart`` MCUs an interval, 0: none; ``scan`` (begin, end) of the entropy-coded
bytes in the stream; ``intervals`` int64 numpy [n, 2]: (begin, end) of every restart interval, markers left out."""
_SOF_NAMES = {0xC1: 'extended sequential (SOF1)', 0xC2: 'progressive (SOF2)', 0xC3: 'lossless (SOF3)', 0xC5: 'differential sequential (SOF5)',
              0xC6: 'differential progressive (SOF6)', 0xC7: 'differential lossless (SOF7)', 0xC9: 'arithmetic coding (SOF9)', 0xCA: 'arithmetic coding (SOF10)',
              0xCB: 'arithmetic coding (SOF11)', 0xCD: 'arithmetic coding (SOF13)', 0xCE: 'arithmetic coding (SOF14)', 0xCF: 'arithmetic coding (SOF15)',
              0xCC: 'arithmetic coding (DAC)'}


def _check_dht(bits, values, what='jpeg_decode_tables'):
    bits, values = tuple(int(b) for b in bits), tuple(int(v) for v in values)
    if len(bits) != 16 or min(bits) < 0 or sum(bits) != len(values) or any(not 0 <= v <= 255 for v in values):
        raise ValueError(f'{what}: a Huffman table is 16 counts and as many symbols 0 .. 255 as they add up to')
    if len(values) > 256:
        raise ValueError(f'{what}: a Huffman table lists {len(values)} symbols, more than 256')
    if sum(n << (16 - length) for length, n in enumerate(bits, start=1)) > 1 << 16:
        raise ValueError(f'{what}: the counts {bits} over-subscribe the code space')
    return bits, values


_decode_tables = {}


def jpeg_decode_tables(bits, values):
    """int32 [JPEG_TABLE_WORDS] on the host (the bits of uint32 words): what ``p3d_video_jpeg_unscan`` reads for ONE Huffman table given as a DHT segment
    states it — ``bits``, the number of codes of every length 1 .. 16, and ``values``, the symbols in code order.  The format is p3d_video.h's: a lookup by
    8-bit prefix (length << 16 | symbol, 0: no code that short), then per length the last code + 1 and the index of its first symbol minus its first code
    (Annex F's maxcode and valptr - mincode), then the symbols.  ValueError for counts that over-subscribe the code space or list more than 256 symbols."""
    key = _check_dht(bits, values)
    if key not in _decode_tables:
        bits, values = key
        words = np.zeros(JPEG_TABLE_WORDS, dtype=np.int64)
        lookup = 1 << JPEG_LOOKUP_BITS
        code, k = 0, 0
        for length, n in enumerate(bits, start=1):                                # the canonical assignment of Annex C
            if n:
                words[lookup + length - 1], words[lookup + 16 + length - 1] = code + n, (k - code) & 0xFFFFFFFF
            for i in range(n if length <= JPEG_LOOKUP_BITS else 0):
                shift = JPEG_LOOKUP_BITS - length
                words[(code + i) << shift:(code + i + 1) << shift] = length << 16 | values[k + i]
            code, k = (code + n) << 1, k + n
        for i, v in enumerate(values):
            words[lookup + 32 + (i >> 2)] |= v << (8 * (i & 3))
        _decode_tables[key] = torch.from_numpy(words.astype(np.uint32).view(np.int32))
    return _decode_tables[key]


def jpeg_parse(stream):
    """The ``JpegInfo`` of one JPEG given as ``bytes``: everything ``jpeg_unscan`` and ``jpeg_decode`` need, read from the segments before the scan, and the
    byte range of every restart interval, found by one vectorised search of the scan for 0xFF followed by anything but 0x00 (which is data).  ValueError,
    naming the reason, for what the decoder does not serve — anything but baseline sequential 8-bit Huffman coding (SOF1, progressive, arithmetic), 16-bit
    quantisation tables, 4 components, sampling other than all 1 x 1 or Y 2 x 2 with chroma 1 x 1, more than one scan or a scan that does not interleave
    all components, DNL — and for a stream that is not whole: a header that ends early, a DHT that over-subscribes the code space or lists more than 256
    symbols, RSTm out of the cyclic order 0 .. 7, an interval count other than ceil(n_mcu / interval), any other marker inside the scan, no EOI."""
    if not isinstance(stream, (bytes, bytearray, memoryview)):
        raise ValueError(f'jpeg_parse: stream must be bytes, got {type(stream).__name__}')
    stream = bytes(stream)
    if stream[:2] != b'\xff\xd8':
        raise ValueError('jpeg_parse: not a JPEG: the stream does not begin with SOI')
    at, dqt, dht, frame, restart, scan = 2, {}, {}, None, 0, None
    while scan is None:
        while at + 1 < len(stream) and stream[at] == 0xFF and stream[at + 1] == 0xFF:      # fill bytes before a marker
            at += 1
        if at + 4 > len(stream):
            raise ValueError(f'jpeg_parse: the stream ends inside its header, at byte {at}')
        if stream[at] != 0xFF:
            raise ValueError(f'jpeg_parse: no marker at byte {at} of the header')
        marker, size = stream[at + 1], int.from_bytes(stream[at + 2:at + 4], 'big')
        if marker in _SOF_NAMES:
            raise ValueError(f'jpeg_parse: {_SOF_NAMES[marker]} is not baseline sequential Huffman coding')
        if marker == 0xDC:
            raise ValueError('jpeg_parse: DNL (the height comes after the scan) is not served')
        if marker == 0xD9 or marker == 0xD8 or 0xD0 <= marker <= 0xD7 or marker == 0x01 or marker == 0x00:
            raise ValueError(f'jpeg_parse: the marker 0x{marker:02X} at byte {at} has no place in a header')
        if size < 2 or at + 2 + size > len(stream):
            raise ValueError(f'jpeg_parse: the stream ends inside its header: the segment 0x{marker:02X} at byte {at} runs past the end')
        p = stream[at + 4:at + 2 + size]
        at += 2 + size
        if marker == 0xDB:
            while p:
                if p[0] >> 4:
                    raise ValueError('jpeg_parse: a 16-bit quantisation table (DQT) is not baseline 8-bit')
                if len(p) < 65:
                    raise ValueError('jpeg_parse: a DQT segment ends inside a table')
                dqt[p[0] & 15], p = p[1:65], p[65:]
        elif marker == 0xC4:
            while p:
                if len(p) < 17 or len(p) < 17 + sum(p[1:17]):
                    raise ValueError('jpeg_parse: a DHT segment ends inside a table')
                n = sum(p[1:17])
                dht[p[0]], p = _check_dht(p[1:17], p[17:17 + n], 'jpeg_parse: DHT'), p[17 + n:]
        elif marker == 0xC0:
            if frame is not None:
                raise ValueError('jpeg_parse: a second SOF0')
            if len(p) < 6 or len(p) != 6 + 3 * p[5]:
                raise ValueError('jpeg_parse: SOF0 has the wrong length')
            if p[0] != 8:
                raise ValueError(f'jpeg_parse: {p[0]}-bit samples are not baseline 8-bit')
            if p[5] == 4:
                raise ValueError('jpeg_parse: 4 components (CMYK / YCCK) are not served')
            if p[5] not in (1, 3):
                raise ValueError(f'jpeg_parse: {p[5]} components: 1 (grey) or 3 (Y Cb Cr) are served')
            frame = (int.from_bytes(p[1:3], 'big'), int.from_bytes(p[3:5], 'big'), [tuple(p[6 + 3 * i:9 + 3 * i]) for i in range(p[5])])
            if frame[0] == 0:
                raise ValueError('jpeg_parse: a height of 0 leaves it to DNL, which is not served')
            if frame[1] == 0:
                raise ValueError('jpeg_parse: a width of 0')
        elif marker == 0xDD:
            if len(p) != 2:
                raise ValueError('jpeg_parse: DRI has the wrong length')
            restart = int.from_bytes(p, 'big')
        elif marker == 0xDA:
            if frame is None:
                raise ValueError('jpeg_parse: SOS before SOF0')
            scan = p
    h, w, components = frame
    nc = len(components)
    if not scan or len(scan) != 4 + 2 * scan[0]:
        raise ValueError('jpeg_parse: SOS has the wrong length')
    if scan[0] != nc or [scan[1 + 2 * i] for i in range(nc)] != [c[0] for c in components]:
        raise ValueError(f'jpeg_parse: the scan holds {scan[0]} of {nc} components: more than one scan, or a scan that is not interleaved, is not served')
    if tuple(scan[1 + 2 * nc:]) != (0, 63, 0):
        raise ValueError('jpeg_parse: the scan is not the whole band 0 .. 63 at full precision: not baseline sequential')
    sampling = [c[1] for c in components]
    if nc == 1 or sampling == [0x11, 0x11, 0x11]:                                     # (one component: its sampling factors play no part, T.81 A.2.2)
        subsampling = '4:4:4'
    elif sampling == [0x22, 0x11, 0x11]:
        subsampling = '4:2:0'
    else:
        raise ValueError(f'jpeg_parse: sampling factors {" ".join(f"{s >> 4}x{s & 15}" for s in sampling)}: all 1x1 (4:4:4) or Y 2x2 with chroma 1x1 (4:2:0) are served')
    selected = []
    for i, c in enumerate(components):
        tdta = scan[2 + 2 * i]
        if c[2] not in dqt or (tdta >> 4) not in dht or (0x10 | (tdta & 15)) not in dht:
            raise ValueError(f'jpeg_parse: component {c[0]} selects a table the stream does not define')
        selected.append((bytes(dqt[c[2]]), dht[tdta >> 4], dht[0x10 | (tdta & 15)]))
    if nc == 3 and selected[1] != selected[2]:
        raise ValueError('jpeg_parse: Cb and Cr select different tables: one chroma set is served')
    luma, chroma = selected[0], selected[-1]
    tables = tuple(torch.tensor(list(t[0]), dtype=torch.uint8) for t in (luma, chroma))
    huffman = (luma[1], chroma[1], luma[2], chroma[2])

    body = np.frombuffer(stream, dtype=np.uint8, offset=at)
    markers = np.flatnonzero((body[:-1] == 0xFF) & (body[1:] != 0)) if body.shape[0] > 1 else np.zeros([0], dtype=np.int64)
    kinds = body[markers + 1]
    others = np.flatnonzero((kinds < 0xD0) | (kinds > 0xD7))
    if others.shape[0] == 0:
        raise ValueError('jpeg_parse: the scan has no EOI')
    last = int(others[0])
    if kinds[last] != 0xD9:
        reason = {0xDA: 'a second scan (SOS)', 0xDC: 'DNL', 0xC4: 'tables (DHT) for a second scan', 0xFF: 'a fill byte (0xFF 0xFF)'}.get(int(kinds[last]), 'a marker')
        raise ValueError(f'jpeg_parse: {reason}, 0xFF 0x{int(kinds[last]):02X}, inside the scan at byte {at + int(markers[last])}: only RSTm and EOI are served')
    rst, end = markers[:last], int(markers[last])
    if not np.array_equal(kinds[:last] - 0xD0, np.arange(last) & 7):
        raise ValueError(f'jpeg_parse: the restart markers are out of the cyclic order 0 .. 7: {[int(k) - 0xD0 for k in kinds[:last]][:16]}')
    _, n_mcu, _, _ = jpeg_layout(h, w, subsampling)
    expected = -(-n_mcu // restart) if restart else 1
    if last + 1 != expected:
        raise ValueError(f'jpeg_parse: {last + 1} restart intervals, but {n_mcu} MCUs at an interval of {restart} make {expected}')
    intervals = at + np.stack([np.concatenate([[0], rst + 2]), np.concatenate([rst, [end]])], axis=1).astype(np.int64)
    return JpegInfo(h, w, subsampling, nc, tables, huffman, restart, (at, at + end), intervals)


def _jpeg_unscan_numpy(data, ranges, tables, table_of_frame, n_mcu, bpm, coded, restart):
    """The rules of p3d_video.h with every interval a row of numpy arrays: one step decodes ONE coefficient (a symbol and its extra bits) of every interval
    still running.  ``data`` uint8 [n], ``ranges`` int64 [F, n_intervals, 2], ``tables`` [n_sets, 4, JPEG_TABLE_WORDS] as uint32 values in int64."""
    f, n_intervals = ranges.shape[:2]
    lanes = f * n_intervals
    begin = np.clip(ranges[..., 0].reshape(-1), 0, data.shape[0])
    end = np.clip(ranges[..., 1].reshape(-1), begin, data.shape[0])
    # the data bytes of every interval — a 0x00 straight after a 0xFF of the interval dropped — each interval followed by 8 zero bytes: the bits past its end
    n_raw = end - begin
    start = np.cumsum(n_raw) - n_raw
    lane_of = np.repeat(np.arange(lanes), n_raw)
    raw = data[np.arange(int(n_raw.sum())) - start[lane_of] + begin[lane_of]].astype(np.int64)
    first = np.zeros(raw.shape[0], dtype=bool)
    first[start[n_raw > 0]] = True
    keep = ~((raw == 0) & np.concatenate([[False], raw[:-1] == 0xFF]) & ~first)
    lane_of = lane_of[keep]
    n_bytes = np.bincount(lane_of, minlength=lanes)
    base = np.cumsum(n_bytes + 8) - (n_bytes + 8)
    padded = np.zeros(int((n_bytes + 8).sum()), dtype=np.int64)
    padded[base[lane_of] + np.arange(lane_of.shape[0]) - (np.cumsum(n_bytes) - n_bytes)[lane_of]] = raw[keep]
    total = 8 * n_bytes

    frame, interval = np.arange(lanes) // n_intervals, np.arange(lanes) % n_intervals
    mcu0 = interval * restart
    n_blocks = np.minimum(restart, n_mcu - mcu0) * coded
    table_base = np.clip(table_of_frame[frame], 0, tables.shape[0] - 1) * 4 * JPEG_TABLE_WORDS
    words = tables.reshape(-1)
    lookup, longer = 1 << JPEG_LOOKUP_BITS, np.arange(JPEG_LOOKUP_BITS + 1, 17)
    bit, block, z = np.zeros(lanes, dtype=np.int64), np.zeros(lanes, dtype=np.int64), np.zeros(lanes, dtype=np.int64)
    pred, status = np.zeros([lanes, 3], dtype=np.int64), np.zeros(lanes, dtype=np.int64)
    out = np.zeros(f * n_mcu * bpm * 64, dtype=np.int16)

    def peek(a, at):                                                              # the 16 bits from bit ``at`` of the lanes ``a``
        i = base[a] + (at >> 3)
        return ((padded[i] << 16 | padded[i + 1] << 8 | padded[i + 2]) >> (8 - (at & 7))) & 0xFFFF
    a = np.flatnonzero(n_blocks > 0)
    while a.shape[0]:
        k = block[a] % coded
        comp = k if bpm == 3 else np.maximum(k - 3, 0)
        dc = z[a] == 0
        t = table_base[a] + (np.where(dc, 0, 2) + (comp > 0)) * JPEG_TABLE_WORDS
        bits = peek(a, bit[a])
        entry = words[t + (bits >> (16 - JPEG_LOOKUP_BITS))]
        length, symbol = entry >> 16, entry & 255
        no_code = np.zeros(a.shape[0], dtype=bool)
        slow = np.flatnonzero((length < 1) | (length > JPEG_LOOKUP_BITS))
        if slow.shape[0]:                                                         # Annex F: the first length whose prefix is below the limit
            codes = bits[slow, None] >> (16 - longer)
            hit = codes < words[t[slow, None] + lookup + longer - 1]
            l = hit.argmax(axis=1)
            offset = words[t[slow] + lookup + 16 + longer[l] - 1]
            at = codes[np.arange(slow.shape[0]), l] + np.where(offset >= 1 << 31, offset - (1 << 32), offset)
            found = hit.any(axis=1) & (at >= 0) & (at < 256)
            at = np.clip(at, 0, 255)
            length[slow] = np.where(found, longer[l], 16)
            symbol[slow] = (words[t[slow] + lookup + 32 + (at >> 2)] >> (8 * (at & 3))) & 255
            no_code[slow] = ~found
        flags = np.where(no_code, JPEG_STATUS['NO_CODE'], 0)
        bit_after = bit[a] + length
        flags |= np.where(bit_after > total[a], JPEG_STATUS['EXHAUSTED'], 0)
        size, run = np.where(dc, symbol, symbol & 15), np.where(dc, 0, symbol >> 4)
        eob, zrl = ~dc & (size == 0) & (run == 0), ~dc & (size == 0) & (run == 15)
        bad = np.where(dc, size > 11, (size > 10) | ((size == 0) & ~eob & ~zrl))
        flags = np.where((flags == 0) & bad, JPEG_STATUS['SIZE'], flags)
        size = np.where(flags == 0, size, 0)
        extra = peek(a, bit_after) >> (16 - size)
        bit_after = bit_after + size
        flags = np.where((flags == 0) & (bit_after > total[a]), JPEG_STATUS['EXHAUSTED'], flags)
        value = np.where(size == 0, 0, np.where(extra >= (1 << np.maximum(size - 1, 0)), extra, extra - (1 << size) + 1))
        position = np.where(dc | eob, z[a], z[a] + np.where(zrl, 16, run))
        flags = np.where((flags == 0) & (position > 63), JPEG_STATUS['RUN'], flags)
        good = flags == 0
        status[a] |= flags
        value = np.where(dc, np.clip(pred[a, comp] + value, -32768, 32767), value)
        store = good & ~eob & ~zrl
        lane = a[store]
        pred[lane[dc[store]], comp[store][dc[store]]] = value[store][dc[store]]
        out[(((frame[lane] * n_mcu + mcu0[lane] + block[lane] // coded) * bpm + k[store]) * 64 + position[store])] = value[store]
        position = np.where(eob, 64, np.where(zrl, position, position + 1))
        done = position > 63                                                      # the block is complete
        bit[a], z[a] = bit_after, np.where(done, 0, position)
        block[a] += done
        finished = good & done & (block[a] == n_blocks[a])
        status[a[finished]] |= np.where((total[a[finished]] - bit[a[finished]]) >> 3 > 1, JPEG_STATUS['LEFTOVER'], 0)
        a = a[good & ~finished]
    return out.reshape(f, n_mcu, bpm, 64), status.reshape(f, n_intervals).astype(np.int32)


def _annex_k_decode_tables():
    return (torch.stack([jpeg_decode_tables(*t) for t in _ANNEX_K])[None],)


def jpeg_unscan(data, ranges, h, w, subsampling='4:2:0', tables=None, table_of_frame=None, restart=JPEG_RESTART, components=3):
    """``(coefficients int16 [F, n_mcu, 3 or 6, 64], status int32 [F, n_intervals])``: the inverse of ``jpeg_scan`` — and of any baseline coder that cuts its
    scans into restart intervals.  ``data`` uint8 [n]: the bytes of all scans; ``ranges`` int64 [F, n_intervals, 2]: the (begin, end) of every interval of
    every frame in ``data``, markers left out (``jpeg_parse``'s ``intervals``, shifted to where the scan went), with n_intervals = ceil(n_mcu / restart);
    ``restart`` 0 means none: one interval of the whole frame.  ``tables`` int32 [n_sets, 4, JPEG_TABLE_WORDS]: sets of ``jpeg_decode_tables`` in the order DC
    luma, DC chroma, AC luma, AC chroma — optimised tables differ from file to file — and ``table_of_frame`` int32 [F] the set of every frame; by default the
    Annex K tables of ``jpeg_scan`` for all.  ``components`` 1: grey streams, laid out as 4:4:4 with zero chroma blocks.  The coefficients are in
    ``jpeg_coefficients``' layout, so ``jpeg_decode`` takes them as they are.  ``status`` is 0 for an interval that decoded cleanly, else the ``JPEG_STATUS``
    bits that stopped it — what it had decoded stays, the rest of it is zero, and no other interval is touched.  Device tensors: one asynchronous fill and
    ONE launch of ``p3d_video_jpeg_unscan``, a lane per interval, and no synchronisation; CPU tensors: the numpy formulation.  The parallel unit is the
    interval: a stream without restart markers is one lane a frame — correct, but slow (DESIGN.md section 2.1y has the figures)."""
    sub = _check_subsampling(subsampling)
    h, w = int(h), int(w)
    _, n_mcu, bpm, _ = jpeg_layout(h, w, sub)
    if components not in (1, 3) or (components == 1 and sub):
        raise ValueError(f'jpeg_unscan: components is 3, or 1 at 4:4:4, got {components!r} at subsampling {subsampling!r}')
    if isinstance(restart, bool) or int(restart) != restart or int(restart) < 0:
        raise ValueError(f'jpeg_unscan: restart must be an integer >= 0, got {restart!r}')
    restart = min(int(restart), n_mcu) or n_mcu
    n_intervals = -(-n_mcu // restart) if n_mcu else 0
    if not torch.is_tensor(data) or data.dtype != torch.uint8 or data.ndim != 1:
        raise ValueError('jpeg_unscan: data must be a uint8 [n] tensor')
    device = data.device
    if not torch.is_tensor(ranges) or ranges.dtype != torch.int64 or ranges.ndim != 3 or ranges.shape[2] != 2:
        raise ValueError('jpeg_unscan: ranges must be an int64 [F, n_intervals, 2] tensor')
    f = ranges.shape[0]
    if h < 0 or w < 0 or f * h * w >= MAX_PIXELS:
        raise ValueError(f'jpeg_unscan: {f} x {h} x {w} pixels are negative or reach 2^31')
    if f * h * w == 0:
        return torch.zeros([f, 0, bpm, 64], dtype=torch.int16, device=device), torch.zeros([f, 0], dtype=torch.int32, device=device)
    if ranges.shape[1] != n_intervals:
        raise ValueError(f'jpeg_unscan: {n_mcu} MCUs at an interval of {restart} are {n_intervals} intervals a frame, got ranges for {ranges.shape[1]}')
    if tables is None:
        tables, = _device_tables('decode tables', device, _annex_k_decode_tables)
    if not torch.is_tensor(tables) or tables.dtype != torch.int32 or tables.ndim != 3 or tuple(tables.shape[1:]) != (4, JPEG_TABLE_WORDS) or tables.shape[0] < 1:
        raise ValueError(f'jpeg_unscan: tables must be an int32 [n_sets, 4, {JPEG_TABLE_WORDS}] tensor')
    if table_of_frame is None:
        table_of_frame = torch.zeros([f], dtype=torch.int32, device=device)
    if not torch.is_tensor(table_of_frame) or table_of_frame.dtype != torch.int32 or tuple(table_of_frame.shape) != (f,):
        raise ValueError(f'jpeg_unscan: table_of_frame must be an int32 [{f}] tensor')
    if not data.is_cuda:
        out, status = _jpeg_unscan_numpy(data.contiguous().numpy(), ranges.cpu().numpy(), tables.cpu().contiguous().numpy().view(np.uint32).astype(np.int64),
                                         table_of_frame.cpu().numpy().astype(np.int64), n_mcu, bpm, 1 if components == 1 else bpm, restart)
        return torch.from_numpy(out), torch.from_numpy(status)
    data, ranges, tables, table_of_frame = (t.to(device).contiguous() for t in (data, ranges, tables, table_of_frame))
    out = torch.empty([f, n_mcu, bpm, 64], dtype=torch.int16, device=device)
    status = torch.empty([f, n_intervals], dtype=torch.int32, device=device)
    with _lib.kernel_timer('video_jpeg_unscan', out):
        code = video_lib().p3d_video_jpeg_unscan(_lib.ptr(data), data.shape[0], _lib.ptr(ranges), _lib.ptr(tables), tables.shape[0], _lib.ptr(table_of_frame),
                                                 f, h, w, sub, int(components), restart, _lib.ptr(out), _lib.ptr(status), _lib.stream_of(out))
    check(code, 'video_jpeg_unscan')
    return out, status


def _upload(array, device):
    """A host array on ``device`` without a wait: through pinned memory, which the copy may leave behind it."""
    t = torch.from_numpy(np.ascontiguousarray(array))
    return t.pin_memory().to(device, non_blocking=True) if torch.device(device).type == 'cuda' else t


def jpeg_status_names(bits):
    """The names of the ``JPEG_STATUS`` bits set in ``bits``."""
    return [name for name, bit in JPEG_STATUS.items() if int(bits) & bit]


def decode_jpeg(streams, device=None, errors='raise'):
    """uint8 [F, H, W, 3] on ``device`` (default: the host): the pictures of a list of baseline JPEG ``bytes`` of ONE size — ours (``encode_jpeg``, the frames
    of ``read_avi``) or anybody's that ``jpeg_parse`` accepts; grey streams show r = g = b.  The headers are parsed on the host, the scans go to the device
    in ONE copy, the frames are grouped by geometry (subsampling, restart interval) for ``jpeg_unscan`` — a fill and a launch a group — and every run of
    frames with equal quantisation tables is one ``jpeg_decode`` (two launches) into its rows of the result.  What ``jpeg_decode`` shows for our own streams
    is ``jpeg_reconstruct`` of the frames they were made from, byte for byte; against libjpeg's decoder a level here and there differs.
    ``errors='raise'``: a scan that does not decode cleanly is a ValueError naming frame, interval and reason — one small device -> host copy.
    ``errors='status'``: ``(frames, status)`` with status int32 [F, the most intervals of a frame] (``JPEG_STATUS`` bits, 0: clean or no such interval) on the
    device, and no synchronisation; a damaged interval shows what it decoded and zeros (grey) after it."""
    if errors not in ('raise', 'status'):
        raise ValueError(f"decode_jpeg: errors is 'raise' or 'status', got {errors!r}")
    device = torch.device('cpu' if device is None else device)
    infos = [jpeg_parse(s) for s in streams]
    if not infos:
        raise ValueError('decode_jpeg: no stream')
    h, w = infos[0].h, infos[0].w
    for i, info in enumerate(infos):
        if (info.h, info.w) != (h, w):
            raise ValueError(f'decode_jpeg: stream {i} is {info.h} x {info.w}, stream 0 {h} x {w}: one call, one size')
    f = len(infos)
    if f * h * w >= MAX_PIXELS:
        raise ValueError(f'decode_jpeg: {f} x {h} x {w} pixels reach 2^31')
    sizes = np.array([0] + [info.scan[1] - info.scan[0] for info in infos], dtype=np.int64)
    offsets = np.cumsum(sizes)
    data = _upload(np.frombuffer(bytearray().join(s[info.scan[0]:info.scan[1]] for s, info in zip(streams, infos)), dtype=np.uint8), device)
    sets, quant = {}, {}                                                          # the distinct Huffman sets and quantisation pairs, in order of appearance
    set_of = [sets.setdefault(info.huffman, len(sets)) for info in infos]
    quant_of = [quant.setdefault(tuple(bytes(t.tolist()) for t in info.tables), len(quant)) for info in infos]
    tables = _upload(torch.stack([torch.stack([jpeg_decode_tables(*t) for t in key]) for key in sets]).numpy(), device)
    quant_tables = _upload(np.array([[list(t) for t in key] for key in quant], dtype=np.uint8), device)
    frames = torch.empty([f, h, w, 3], dtype=torch.uint8, device=device)
    status = torch.zeros([f, max(info.intervals.shape[0] for info in infos)], dtype=torch.int32, device=device)
    groups = {}
    for i, info in enumerate(infos):
        groups.setdefault((info.subsampling, info.components, info.restart), []).append(i)
    for (subsampling, components, restart), members in groups.items():
        ranges = _upload(np.stack([infos[i].intervals - infos[i].scan[0] + offsets[i] for i in members]), device)
        table_of_frame = _upload(np.array([set_of[i] for i in members], dtype=np.int32), device)
        coefficients, group_status = jpeg_unscan(data, ranges, h, w, subsampling, tables, table_of_frame, restart, components)
        whole = members == list(range(f))                                         # the usual case: one group
        if whole:
            status[:, :group_status.shape[1]] = group_status
        else:
            status[_upload(np.array(members), device), :group_status.shape[1]] = group_status
        a = 0
        while a < len(members):                                                   # runs of frames that are neighbours in the result and share their tables
            b = a + 1
            while b < len(members) and members[b] == members[b - 1] + 1 and quant_of[members[b]] == quant_of[members[a]]:
                b += 1
            jpeg_decode(coefficients[a:b], quant_tables[quant_of[members[a]]], h, w, subsampling, out=frames[members[a]:members[a] + b - a])
            a = b
    if errors == 'status':
        return frames, status
    bad = status.cpu().nonzero()
    if bad.shape[0]:
        i, j = bad[0].tolist()
        raise ValueError(f'decode_jpeg: frame {i}, restart interval {j} does not decode: {", ".join(jpeg_status_names(status[i, j]))}'
                         f' ({bad.shape[0]} damaged interval{"s" if bad.shape[0] > 1 else ""} in all)')
    return frames


def load_jpeg(path, device=None):
    """uint8 [H, W, 3] on ``device``: the picture of a baseline JPEG file (``decode_jpeg``)."""
    with open(path, 'rb') as fh:
        return decode_jpeg([fh.read()], device)[0]
