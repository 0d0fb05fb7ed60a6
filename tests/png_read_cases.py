"""Shared by test_video_png_read_host.py / test_video_png_read_gpu.py: an inflate from first principles (a plain loop, one bit at a time, codes kept as
strings of '0' and '1' — nothing of pix2pix3d_amd.video's decode path), the streams the tests read (our own writer's, Pillow's, raw zlib's, and damaged
ones), and the case file of tools/png_inflate_check.cpp.  Everything is made once and only read."""
import io
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import torch

import png_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# p3d_video.h: P3D_VIDEO_PNG_STATUS_*
BLOCK_TYPE, STORED, CODE_LENGTHS, NO_CODE, DISTANCE, OVERFLOW, EXHAUSTED, LEFTOVER, BOUNDARY, SHORT, FILTER, ADLER = (1 << i for i in range(12))
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
_made = {}


# ---- inflate from first principles -------------------------------------------------------------------------------------------------------------------
def code_strings(lengths):
    """{'0101': symbol} of the canonical code (RFC 1951 section 3.2.2), or None where the lengths over-subscribe the code space."""
    if sum(2.0 ** -l for l in lengths if l) > 1:
        return None
    table, code = {}, 0
    for bits in range(1, 16):
        for s, l in enumerate(lengths):
            if l == bits:
                table[format(code, f'0{bits}b')] = s
                code += 1
        code *= 2
    return table


def reference_part(raw, room, final):
    """(the bytes written, status) of ONE part whose bytes are ``raw`` and whose output range holds ``room`` bytes, under p3d_video.h's rules."""
    state = {'at': 0, 'status': 0}
    out = []

    def bit():
        at = state['at']
        state['at'] = at + 1
        if at >= 8 * len(raw):
            state['status'] |= EXHAUSTED
            return 0
        return (raw[at >> 3] >> (at & 7)) & 1

    def bits(n):
        return sum(bit() << i for i in range(n))

    def symbol(table):
        code = ''
        for _ in range(15):
            code += str(bit())
            if code in table:
                return table[code]
        state['status'] |= NO_CODE
        return None

    def put(v):
        if len(out) >= room:
            state['status'] |= OVERFLOW
            return False
        out.append(v)
        return True

    def tables(kind):
        if kind == 1:
            return code_strings([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), code_strings([5] * 32)
        n_lit, n_dist, n_cl = bits(5) + 257, bits(5) + 1, bits(4) + 4
        if state['status']:
            return None
        if n_lit > 286 or n_dist > 30:
            state['status'] |= CODE_LENGTHS
            return None
        cl = [0] * 19
        for s in CL_ORDER[:n_cl]:
            cl[s] = bits(3)
        if state['status']:
            return None
        cl = code_strings(cl)
        lengths = []
        while cl is not None and len(lengths) < n_lit + n_dist:
            v = symbol(cl)
            if state['status']:
                return None
            if v < 16:
                lengths.append(v)
                continue
            if v == 16 and not lengths:
                break
            value = lengths[-1] if v == 16 else 0
            repeat = 3 + bits(2) if v == 16 else 3 + bits(3) if v == 17 else 11 + bits(7)
            if state['status']:
                return None
            lengths += [value] * repeat
        lit = code_strings(lengths[:n_lit]) if len(lengths) == n_lit + n_dist else None
        dist = code_strings(lengths[n_lit:]) if lit is not None else None
        if dist is None:
            state['status'] |= CODE_LENGTHS
            return None
        return lit, dist

    def decode():
        while True:
            last, kind = bit(), bits(2)
            if state['status']:
                return
            if kind == 3:
                state['status'] |= BLOCK_TYPE
                return
            if last and not final:
                state['status'] |= BOUNDARY
                return
            if kind == 0:
                while state['at'] & 7:
                    bit()
                n, complement = bits(16), bits(16)
                if state['status']:
                    return
                if n != complement ^ 0xFFFF:
                    state['status'] |= STORED
                    return
                for _ in range(n):
                    v = bits(8)
                    if state['status'] or not put(v):
                        return
            else:
                both = tables(kind)
                if state['status']:
                    return
                lit, dist = both
                while True:
                    v = symbol(lit)
                    if state['status']:
                        return
                    if v == 256:
                        break
                    if v < 256:
                        if not put(v):
                            return
                        continue
                    if v >= 286:
                        state['status'] |= NO_CODE
                        return
                    length = png_cases.LENGTH_BASE[v - 257] + bits(png_cases.LENGTH_EXTRA[v - 257])
                    if state['status']:
                        return
                    d = symbol(dist)
                    if state['status']:
                        return
                    if d >= 30:
                        state['status'] |= NO_CODE
                        return
                    distance = DIST_BASE[d] + bits(DIST_EXTRA[d])
                    if state['status']:
                        return
                    if distance > len(out):
                        state['status'] |= DISTANCE
                        return
                    for _ in range(length):
                        if not put(out[-distance]):
                            return
            if last if final else state['at'] == 8 * len(raw):
                break
        if final and (8 * len(raw) - state['at']) // 8 > 0:
            state['status'] |= LEFTOVER
        if len(out) < room:
            state['status'] |= SHORT
    decode()
    return bytes(out), state['status']


def reference_inflate(data, parts, out_bytes):
    """(bytes [out_bytes], [status]) of a case by ``reference_part``, the ranges clamped as the entry point clamps them."""
    raw, out, status = bytes(data.tolist()), bytearray(out_bytes), []
    for in_begin, in_end, out_begin, out_end, final in parts.tolist():
        in_begin = min(max(in_begin, 0), len(raw))
        in_end = min(max(in_end, in_begin), len(raw))
        out_begin = min(max(out_begin, 0), out_bytes)
        out_end = min(max(out_end, out_begin), out_bytes)
        written, s = reference_part(raw[in_begin:in_end], out_end - out_begin, bool(final))
        out[out_begin:out_begin + len(written)] = written
        status.append(s)
    return bytes(out), status


# ---- files --------------------------------------------------------------------------------------------------------------------------------------------
def chunk(kind, payload):
    return len(payload).to_bytes(4, 'big') + kind + payload + zlib.crc32(kind + payload).to_bytes(4, 'big')


def chunks_of(stream):
    """[(type, payload)] by a plain walk, CRCs not looked at."""
    at, out = 8, []
    while at < len(stream):
        size = int.from_bytes(stream[at:at + 4], 'big')
        out.append((stream[at + 4:at + 8], stream[at + 8:at + 8 + size]))
        at += 12 + size
    return out


def file_of(chunks):
    return b'\x89PNG\r\n\x1a\n' + b''.join(chunk(k, p) for k, p in chunks)


def replace_chunk(stream, kind, change):
    """The file with the payload of its first chunk ``kind`` replaced by ``change(payload)``, the CRC made anew."""
    chunks, done = [], False
    for k, p in chunks_of(stream):
        if k == kind and not done:
            p, done = change(p), True
        chunks.append((k, p))
    assert done
    return file_of(chunks)


def zlib_of(stream):
    """The zlib stream of a still: its IDAT payloads joined."""
    return b''.join(p for k, p in chunks_of(stream) if k == b'IDAT')


def textured(h=37, w=53, seed=91):
    """uint8 [h, w, 3]: smooth waves plus noise of +-6 — rows that a real encoder turns into one dynamic block with long codes and far matches."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 90 * np.sin(x / 7 + c) * np.cos(y / 5 - c) for c in range(3)], axis=2) + rng.integers(-6, 7, size=[h, w, 3])
    return a.clip(0, 255).astype(np.uint8)


def pillow_png(picture, **settings):
    from PIL import Image
    im = picture if isinstance(picture, Image.Image) else Image.fromarray(picture)
    out = io.BytesIO()
    im.save(out, 'PNG', **settings)
    return out.getvalue()


def pillow_pixels(stream):
    """The file's pixels in ``decode_png``'s layout, PIL the decoder: 'I;16' as big-endian byte pairs, 'P' the indices."""
    from PIL import Image
    with Image.open(io.BytesIO(stream)) as im:
        im.load()
        a = np.asarray(im)
        if im.mode.startswith('I'):
            a = a.astype(np.int64)
            return np.stack([a >> 8, a & 255], axis=2).astype(np.uint8)
        return a.copy()


def pillow_files():
    """{label: PNG bytes} as Pillow writes them."""
    if 'pillow' not in _made:
        from PIL import Image
        rng = np.random.default_rng(92)
        rgb = textured()
        flat = np.full([20, 300, 3], 200, dtype=np.uint8)
        noise = rng.integers(0, 256, size=[300, 300, 3], dtype=np.uint8)
        grey16 = (rgb[..., 0].astype(np.uint16) * 257 + rng.integers(0, 200, size=rgb.shape[:2])).astype(np.uint16)
        _made['pillow'] = {
            'RGB default': pillow_png(rgb), 'RGB optimize': pillow_png(rgb, optimize=True), 'RGB level 1': pillow_png(rgb, compress_level=1),
            'RGB level 0': pillow_png(rgb, compress_level=0), 'flat': pillow_png(flat), 'noise, 5 IDAT': pillow_png(noise),
            'L': pillow_png(rgb[..., 0]), 'LA': pillow_png(Image.merge('LA', [Image.fromarray(rgb[..., 0].copy()), Image.fromarray(rgb[..., 1].copy())])), 'RGBA': pillow_png(np.concatenate([rgb, rgb[..., :1]], axis=2)),
            'P 256': pillow_png(Image.fromarray(rgb).quantize(256)), 'I;16': pillow_png(Image.fromarray(grey16))}
    return _made['pillow']


def own_files():
    """[(label, mode, frames, palette, index, [PNG bytes])]: ``encode_png`` of png_cases.mode_frames in all six modes with and without the index, of the
    Fibonacci frame (codes of 15 bits; 71 segments) and of a frame of three segments."""
    if 'own' not in _made:
        from pix2pix3d_amd import video
        out = []
        for index in (False, True):
            for mode in png_cases.MODES:
                frames, palette = png_cases.mode_frames(mode)
                out.append((f'{mode} index={index}', mode, frames, palette, index, video.encode_png(frames, mode, palette, index=index)))
            tall = png_cases.mode_frames('RGB', f=1, h=250, w=100)[0]
            out.append((f'three segments index={index}', 'RGB', tall, None, index, video.encode_png(tall, index=index)))
        fib = png_cases.fibonacci_frame()
        out.append(('fibonacci index=True', 'L', fib, None, True, video.encode_png(fib, 'L', filter=0, index=True)))
        _made['own'] = out
    return _made['own']


# ---- the cases of png_inflate: (label, data uint8 [n], parts int64 [n_parts, 5], out_bytes, what zlib makes of the stream or None) --------------------------
def case_of(label, stream, firsts=(), rows_bytes=0, out_bytes=None):
    """A case from a zlib stream: one part, or a part per segment where ``firsts`` lists the offsets of all segments but the first and ``rows_bytes`` the
    filtered bytes of a whole segment."""
    want = zlib.decompress(stream[2:-4], -15)                                       # (the raw deflate bytes: a damaged Adler-32 is the reader's business)
    out_bytes = len(want) if out_bytes is None else out_bytes
    cuts = [0] + [o - 2 for o in firsts] + [len(stream) - 6]
    parts = [(cuts[j], cuts[j + 1], j * rows_bytes, min((j + 1) * rows_bytes, out_bytes) if j < len(cuts) - 2 else out_bytes, int(j == len(cuts) - 2))
             for j in range(len(cuts) - 1)]
    return label, torch.tensor(list(stream[2:-4]), dtype=torch.uint8), torch.tensor(parts, dtype=torch.int64), out_bytes, want


def hand_rows(h, n, seed, top=64):
    """bytes of h filtered rows of type 0 with n values below ``top``."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, top, size=[h, 1 + n], dtype=np.uint8)
    rows[:, 0] = 0
    return rows


def far_match_rows():
    """96 rows of 385 bytes, values 0 .. 63, rows 84 .. 95 repeating rows 0 .. 11: matches at a distance of 84 x 385 = 32 340."""
    rows = hand_rows(96, 384, 93)
    rows[84:] = rows[:12]
    return rows.tobytes()


def raw_zlib_streams():
    """{label: zlib stream} straight from zlib: what no PNG writer at hand produces."""
    if 'raw' not in _made:
        small = hand_rows(24, 60, 94).tobytes()
        out = {}
        c = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
        out['fixed block'] = c.compress(small) + c.flush()
        out['two stored blocks'] = zlib.compress(hand_rows(70, 999, 95, top=256).tobytes(), 0)
        c = zlib.compressobj(6, zlib.DEFLATED, 9)
        out['window of 512'] = c.compress(hand_rows(40, 100, 96, top=8).tobytes()) + c.flush()
        out['far match'] = zlib.compress(far_match_rows(), 9)
        _made['raw'] = out
    return _made['raw']


def flushed_stream():
    """(zlib stream, the offset of its second half in it, the bytes before the flush): Z_FULL_FLUSH in the middle — a byte boundary no match crosses."""
    rows = hand_rows(24, 60, 97, top=16).tobytes()
    c = zlib.compressobj(9)
    first = c.compress(rows[:732]) + c.flush(zlib.Z_FULL_FLUSH)
    return first + c.compress(rows[732:]) + c.flush(), len(first), 732


def index_parts(stream):
    """(firsts, the filtered bytes of a segment) of an indexed still of ours, read from its chunks by hand."""
    chunks = dict(chunks_of(stream))
    w, h = int.from_bytes(chunks[b'IHDR'][:4], 'big'), int.from_bytes(chunks[b'IHDR'][4:8], 'big')
    bpp = {(0, 8): 1, (4, 8): 2, (2, 8): 3, (6, 8): 4, (3, 8): 1, (0, 16): 2}[chunks[b'IHDR'][9], chunks[b'IHDR'][8]]
    values = [int.from_bytes(chunks[b'seGM'][i:i + 4], 'big') for i in range(0, len(chunks[b'seGM']), 4)]
    return tuple(values[1:]), values[0] * (1 + w * bpp)


def clean_cases():
    if 'clean' not in _made:
        cases = []
        for label, mode, frames, palette, index, streams in own_files():
            for k, stream in enumerate(streams):
                firsts, rows_bytes = index_parts(stream) if index else ((), 0)
                cases.append(case_of(f'own {label} frame {k}', zlib_of(stream), firsts, rows_bytes))
        cases += [case_of('Pillow ' + label, zlib_of(stream)) for label, stream in pillow_files().items()]
        cases += [case_of('zlib ' + label, stream) for label, stream in raw_zlib_streams().items()]
        stream, second, before = flushed_stream()
        cases.append(case_of('zlib full flush, two parts', stream, (second,), before))
        _made['clean'] = cases
    return _made['clean']


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value, n):                        # least significant bit first: header fields and extra bits
        self.bits += [(value >> i) & 1 for i in range(n)]
        return self

    def code(self, text):                           # a Huffman code, from its most significant bit
        self.bits += [int(c) for c in text]
        return self

    def bytes(self):
        bits = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b << i for i, b in enumerate(bits[k:k + 8])) for k in range(0, len(bits), 8))


def damaged_cases():
    """[(label, data, parts, out_bytes, the status p3d_video.h's rules give)]: each a clean stream with one change."""
    if 'damaged' in _made:
        return _made['damaged']
    cases = []

    def add(label, deflate, out_bytes, status, parts=None):
        parts = [(0, len(deflate), 0, out_bytes, 1)] if parts is None else parts
        cases.append((label, torch.tensor(list(deflate), dtype=torch.uint8), torch.tensor(parts, dtype=torch.int64), out_bytes, status))
    dynamic = zlib_of(pillow_files()['RGB default'])
    n = len(zlib.decompress(dynamic))
    body = bytearray(dynamic[2:-4])
    assert body[0] & 7 == 5                                                        # BFINAL = 1, BTYPE = 2: one dynamic block
    add('a block type of 3', bytes([body[0] | 6]) + bytes(body[1:]), n, [BLOCK_TYPE])
    stored = zlib_of(pillow_files()['RGB level 0'])[2:-4]
    assert stored[0] & 6 == 0
    add('a flipped NLEN bit', stored[:3] + bytes([stored[3] ^ 0x10]) + stored[4:], n, [STORED])
    word = int.from_bytes(body[:8], 'little')
    assert (word >> 13) & 15 >= 0                                                  # HCLEN + 4 >= 4 lengths of 3 bits from bit 17 on: the first four become 1
    word = (word & ~(0xFFF << 17)) | (0b001001001001 << 17)
    add('an over-subscribed header', word.to_bytes(8, 'little') + bytes(body[8:]), n, [CODE_LENGTHS])
    add('a truncated stream', bytes(body[:-5]), n, [EXHAUSTED])
    add('bytes appended', bytes(body) + bytes(3), n, [LEFTOVER])
    add('out_bytes one too small', bytes(body), n - 1, [OVERFLOW])
    add('out_bytes one too large', bytes(body), n + 1, [SHORT])
    # BFINAL = 1, fixed codes; the literal 65 ('00110000' + 65 = 01110001), then length 3 (symbol 257: 0000001) at distance 2 (symbol 1: 00001): one byte too far
    reach = BitWriter().put(1, 1).put(1, 2).code('01110001').code('0000001').code('00001').code('0000000').bytes()
    add('a first match that reaches before the start', reach, 4, [DISTANCE])
    # the same from a part's point of view: the second part of a flushed stream, asked to start where the first did, is sound; a copy of the stream cut
    # one byte late is not a block boundary
    stream, second, before = flushed_stream()
    total = len(zlib.decompress(stream))
    add('a part that is not final meets BFINAL', stream[2:-4], total, [BOUNDARY, 0],
        [(second - 2, len(stream) - 6, 0, total - before, 0), (second - 2, len(stream) - 6, before, total, 1)])
    _made['damaged'] = cases
    return cases


def damaged_files():
    """[(label, PNG bytes, the bits that must be set in the status of frame 0, column 0 — or None where only 'not clean' is certain)]: file-level damage."""
    if 'damaged files' in _made:
        return _made['damaged files']
    from pix2pix3d_amd import video
    out = []
    tall = [streams[0] for label, *_, streams in own_files() if label == 'three segments index=True'][0]

    def moved(p):
        return p[:4] + (int.from_bytes(p[4:8], 'big') + 1).to_bytes(4, 'big') + p[8:]

    def swapped(p):
        assert len(p) == 12 and p[4:8] != p[8:12]                                   # segment_rows and the offsets of the second and the third segment
        return p[:4] + p[8:12] + p[4:8]
    out.append(('an index with one offset moved by a byte', replace_chunk(tall, b'seGM', moved), None))
    out.append(('an index with two offsets swapped', replace_chunk(tall, b'seGM', swapped), None))
    rows = hand_rows(9, 30, 98)
    rows[4, 0] = 7
    header = video.png_header(9, 10, 'RGB')
    out.append(('a filter byte of 7', header + chunk(b'IDAT', zlib.compress(rows.tobytes())) + chunk(b'IEND', b''), FILTER))
    clean = pillow_files()['RGB default']
    out.append(('a flipped Adler byte', replace_chunk(clean, b'IDAT', lambda p: p[:-2] + bytes([p[-2] ^ 1]) + p[-1:]), ADLER))
    _made['damaged files'] = out
    return out


# ---- un-filtering ---------------------------------------------------------------------------------------------------------------------------------------
def filtered_rows(f, h, w, bpp, kind, seed):
    """uint8 [f, h, 1 + w bpp]: random residuals under the forced type ``kind`` 0 .. 4, or 'mix': per row a type in the cycle None, Up, Sub, Average, Paeth —
    so that Paeth stands under Average under Sub."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256, size=[f, h, 1 + w * bpp], dtype=np.uint8)
    rows[:, :, 0] = np.array([0, 2, 1, 3, 4])[np.arange(h) % 5] if kind == 'mix' else kind
    return torch.from_numpy(rows)


def reference_unfilter(rows, bpp):
    """uint8 [h, n] of ONE frame's filtered rows, one byte at a time (the PNG specification's reconstruction functions)."""
    h, n = rows.shape[0], rows.shape[1] - 1
    out = [[0] * n for _ in range(h)]
    for y in range(h):
        kind = int(rows[y, 0])
        kind = kind if kind <= 4 else 0
        for i in range(n):
            a = out[y][i - bpp] if i >= bpp else 0
            b = out[y - 1][i] if y else 0
            c = out[y - 1][i - bpp] if y and i >= bpp else 0
            if kind == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            else:
                pred = (0, a, b, (a + b) // 2)[kind]
            out[y][i] = (int(rows[y, 1 + i]) + pred) % 256
    return np.array(out, dtype=np.uint8).reshape(h, n)


# ---- the case file of tools/png_inflate_check.cpp --------------------------------------------------------------------------------------------------------
def write_case_file(path, cases):
    with open(path, 'wb') as fh:
        fh.write(b'PIC1' + struct.pack('<i', len(cases)))
        for _, data, parts, out_bytes, _ in cases:
            fh.write(struct.pack('<3q', data.shape[0], out_bytes, parts.shape[0]))
            fh.write(parts.contiguous().numpy().tobytes())
            fh.write(data.contiguous().numpy().tobytes())


def read_results(path, cases):
    """[(out uint8 [out_bytes], status int32 [n_parts])] as the stand-alone program wrote them."""
    raw, at, out = open(path, 'rb').read(), 0, []
    for _, _, parts, out_bytes, _ in cases:
        n = parts.shape[0]
        out.append((torch.from_numpy(np.frombuffer(raw, dtype=np.uint8, count=out_bytes, offset=at).copy()),
                    torch.from_numpy(np.frombuffer(raw, dtype=np.int32, count=n, offset=at + out_bytes).copy())))
        at += out_bytes + 4 * n
    assert at == len(raw)
    return out


def build_checker(directory, sanitize=True):
    """(path of the stand-alone inflate built from tools/png_inflate_check.cpp, whether it carries the sanitizers).  A host compiler only: no HIP, no
    Python.  Where no compiler links the sanitizer runtimes, the plain build — and False."""
    from pix2pix3d_amd import build
    source, include = os.path.join(ROOT, 'tools', 'png_inflate_check.cpp'), os.path.join(build.CSRC, 'video')
    compilers = [c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++')) if c]
    attempts = [(c, True) for c in compilers if sanitize] + [(c, False) for c in compilers]
    log = []
    for compiler, sanitized in attempts:
        exe = os.path.join(directory, 'png_inflate_check' + ('_san' if sanitized else ''))
        flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-O1', '-g'] if sanitized else ['-O2']
        r = subprocess.run([compiler, '-std=c++17', '-Wall', *flags, '-I', include, source, '-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode == 0:
            return exe, sanitized
        log.append(f'{compiler} {" ".join(flags)}:\n{r.stdout}')
    raise AssertionError('no host compiler built tools/png_inflate_check.cpp:\n' + '\n'.join(log))


def run_checker(exe, cases, directory):
    """The results of the stand-alone program on ``cases``; it must end with status 0 and nothing on stderr (a sanitizer report is both)."""
    case_file, result_file = os.path.join(directory, 'png_cases.bin'), os.path.join(directory, 'png_results.bin')
    write_case_file(case_file, cases)
    r = subprocess.run([exe, case_file, result_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == '', (r.returncode, r.stdout, r.stderr)
    return read_results(result_file, cases)
