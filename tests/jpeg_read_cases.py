"""Shared by test_video_jpeg_read_host.py / test_video_jpeg_read_gpu.py: an entropy DEcoder from first principles (a plain loop, one bit at a time, with its
own canonical-code table from BITS / HUFFVAL — nothing of pix2pix3d_amd.video's decode path), the streams the tests read (our own coder's, Pillow's with its
own tables and restart intervals, and damaged ones), and the case file of tools/jpeg_unscan_check.cpp."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import torch

from jpeg_cases import PICTURES, random_coefficients, split_jpeg, tables_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_CODE, RUN, SIZE, EXHAUSTED, LEFTOVER = 1, 2, 4, 8, 16      # p3d_video.h: P3D_VIDEO_JPEG_STATUS_*


# ---- the entropy decoder from first principles -------------------------------------------------------------------------------------------------
def codes_of(bits, values):
    """(length, code) -> symbol of a DHT's BITS / HUFFVAL (Annex C: codes of one length count up; the next length starts at twice the next code)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[length, code] = values[k]
            code, k = code + 1, k + 1
        code *= 2
    return table


def reference_interval(raw, tables, bpm, coded, n_mcus):
    """(blocks: n_mcus * bpm rows of 64 ints, status) of ONE restart interval's bytes ``raw`` under p3d_video.h's rules.  ``tables``: four (BITS, HUFFVAL) in
    the order DC luma, DC chroma, AC luma, AC chroma; ``coded``: the blocks of an MCU that the stream holds (bpm, or 1 for a grey stream)."""
    data, i = [], 0
    while i < len(raw):                                                           # a 0x00 straight after a 0xFF is stuffing
        data.append(raw[i])
        i += 2 if raw[i] == 0xFF and i + 1 < len(raw) and raw[i + 1] == 0 else 1
    codes = [codes_of(*t) for t in tables]
    state = {'at': 0, 'status': 0}
    blocks = [[0] * 64 for _ in range(n_mcus * bpm)]

    def bit():
        at = state['at']
        state['at'] = at + 1
        if at >= 8 * len(data):
            state['status'] |= EXHAUSTED                                          # past the end: a zero bit, and the status says so
            return 0
        return (data[at >> 3] >> (7 - (at & 7))) & 1

    def symbol(table):
        code = 0
        for length in range(1, 17):
            code = code << 1 | bit()
            if (length, code) in table:
                return table[length, code]
        state['status'] |= NO_CODE
        return None

    def extra(size):
        v = 0
        for _ in range(size):
            v = v << 1 | bit()
        return v if v >= 1 << (size - 1) else v - (1 << size) + 1

    def decode():
        pred = [0, 0, 0]
        for m in range(n_mcus):
            for k in range(coded):
                comp = k if bpm == 3 else max(k - 3, 0)
                block = blocks[m * bpm + k]
                size = symbol(codes[1 if comp else 0])
                if state['status']:
                    return
                if size > 11:
                    state['status'] |= SIZE
                    return
                diff = extra(size) if size else 0
                if state['status']:
                    return
                pred[comp] = min(max(pred[comp] + diff, -32768), 32767)
                block[0] = pred[comp]
                z = 1
                while z <= 63:
                    rs = symbol(codes[3 if comp else 2])
                    if state['status']:
                        return
                    run, size = rs >> 4, rs & 15
                    if size == 0:
                        if run == 0:
                            break
                        if run != 15:
                            state['status'] |= SIZE
                            return
                        z += 16
                        if z > 63:
                            state['status'] |= RUN
                            return
                        continue
                    if size > 10:
                        state['status'] |= SIZE
                        return
                    value = extra(size)
                    if state['status']:
                        return
                    z += run
                    if z > 63:
                        state['status'] |= RUN
                        return
                    block[z] = value
                    z += 1
        if (8 * len(data) - state['at']) // 8 > 1:
            state['status'] |= LEFTOVER
    decode()
    return blocks, state['status']


def header_of(stream):
    """dict(h, w, subsampling, components, restart, quant (luma, chroma: 64 values in zigzag order), huffman (DC luma, DC chroma, AC luma, AC chroma), scan)
    read with jpeg_cases' segment parser; the chroma tables of a grey stream are its luma tables."""
    segments, scan = split_jpeg(stream)
    dqt, dht = tables_of(stream)
    sof, = [p for m, p in segments if m == 0xC0]
    sos, = [p for m, p in segments if m == 0xDA]
    dri = [p for m, p in segments if m == 0xDD]
    assert sof[0] == 8
    h, w, nc = int.from_bytes(sof[1:3], 'big'), int.from_bytes(sof[3:5], 'big'), sof[5]
    comps = [tuple(sof[6 + 3 * i:9 + 3 * i]) for i in range(nc)]
    assert sos[0] == nc
    sel = [sos[2 + 2 * i] for i in range(nc)]
    first, last = 0, nc - 1
    return dict(h=h, w=w, components=nc, subsampling='4:2:0' if nc == 3 and comps[0][1] == 0x22 else '4:4:4', restart=int.from_bytes(dri[-1], 'big') if dri else 0,
                quant=(dqt[comps[first][2]], dqt[comps[last][2]]),
                huffman=(dht[sel[first] >> 4], dht[sel[last] >> 4], dht[0x10 | (sel[first] & 15)], dht[0x10 | (sel[last] & 15)]), scan=scan)


def reference_decode(stream):
    """(coefficients int16 [n_mcu, 3 or 6, 64], the status of every interval, ``header_of(stream)``): the stream's scan cut at its RSTm markers by a plain
    loop, every interval through ``reference_interval``."""
    info = header_of(stream)
    scan = info['scan']
    pieces, begin, i = [], 0, 0
    while i + 1 < len(scan):
        if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7:
            pieces.append(scan[begin:i])
            begin = i = i + 2
        else:
            i += 1
    pieces.append(scan[begin:])
    mcu = 16 if info['subsampling'] == '4:2:0' else 8
    bpm = 6 if info['subsampling'] == '4:2:0' else 3
    n_mcu = -(-info['w'] // mcu) * -(-info['h'] // mcu)
    restart = info['restart'] or n_mcu
    assert len(pieces) == -(-n_mcu // restart), (len(pieces), n_mcu, restart)
    blocks, status = [], []
    for i, piece in enumerate(pieces):
        b, s = reference_interval(piece, info['huffman'], bpm, 1 if info['components'] == 1 else bpm, min(restart, n_mcu - i * restart))
        blocks += b
        status.append(s)
    return np.array(blocks, dtype=np.int64).astype(np.int16).reshape(n_mcu, bpm, 64), status, info


# ---- the streams -------------------------------------------------------------------------------------------------------------------------------
ROUND_TRIPS = {
    # name: (frames, h, w, subsampling, seed) of random_coefficients through jpeg_scan
    'one MCU 4:4:4': (1, 8, 8, '4:4:4', 71), 'one MCU 4:2:0': (1, 16, 16, '4:2:0', 72),
    '19 MCUs 4:4:4': (1, 8, 152, '4:4:4', 73), '19 MCUs 4:2:0': (1, 16, 304, '4:2:0', 74),                  # the last interval holds 3 MCUs
    '81 MCUs 4:4:4': (1, 72, 72, '4:4:4', 75),                                                                # 11 intervals: RSTm wraps past 7
    'three frames 4:2:0': (3, 40, 56, '4:2:0', 76), 'three frames 4:4:4': (3, 24, 40, '4:4:4', 77),
}
FOREIGN_PICTURES = ('gradient', 'noise', 'below one MCU', 'checkerboard')
FOREIGN_SETTINGS = (
    # (mode, Pillow's save arguments)
    ('RGB', dict(quality=50, subsampling=0)),
    ('RGB', dict(quality=90, subsampling=2, optimize=True)),
    ('RGB', dict(quality=90, subsampling=0, optimize=True)),
    ('RGB', dict(quality=90, subsampling=0, restart_marker_blocks=1)),                                         # more than 8 intervals
    ('RGB', dict(quality=50, subsampling=2, restart_marker_blocks=1, optimize=True)),
    ('RGB', dict(quality=90, subsampling=2, restart_marker_blocks=2)),
    ('RGB', dict(quality=50, subsampling=0, restart_marker_rows=1, optimize=True)),
    ('RGB', dict(quality=90, subsampling=2, restart_marker_rows=1)),
    ('L', dict(quality=90)),
    ('L', dict(quality=50, restart_marker_blocks=2, optimize=True)),
)
_made = {}


def round_trip(name):
    """dict(coefficients, data, offsets, h, w, subsampling) of a ROUND_TRIPS row — made once, then only read."""
    if ('round trip', name) not in _made:
        from pix2pix3d_amd import video
        f, h, w, subsampling, seed = ROUND_TRIPS[name]
        _, n_mcu, bpm, _ = video.jpeg_layout(h, w, subsampling)
        coefficients = random_coefficients(f, n_mcu, bpm, seed)
        data, offsets = video.jpeg_scan(coefficients, h, w, subsampling)
        _made['round trip', name] = dict(coefficients=coefficients, data=data, offsets=offsets, h=h, w=w, subsampling=subsampling)
    return _made['round trip', name]


def own_ranges(data, offsets, n_intervals):
    """int64 [F, n_intervals, 2]: the intervals of ``jpeg_scan``'s output, cut at the RSTm markers by a plain loop."""
    raw, ranges = bytes(data.tolist()), []
    for f in range(len(offsets) - 1):
        begin, i, end = int(offsets[f]), int(offsets[f]), int(offsets[f + 1])
        row = []
        while i + 1 < end:
            if raw[i] == 0xFF and 0xD0 <= raw[i + 1] <= 0xD7:
                row.append((begin, i))
                begin = i = i + 2
            else:
                i += 1
        row.append((begin, end))
        assert len(row) == n_intervals
        ranges.append(row)
    return torch.tensor(ranges, dtype=torch.int64)


def pillow_jpeg(picture, mode, **settings):
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(picture).convert(mode).save(out, 'JPEG', **settings)
    return out.getvalue()


def foreign_streams():
    """[(label, stream bytes, mode)]: every FOREIGN_PICTURES x FOREIGN_SETTINGS as Pillow writes it — made once."""
    if 'foreign' not in _made:
        _made['foreign'] = [(f'{name} {mode} {settings}', pillow_jpeg(PICTURES[name], mode, **settings), mode)
                            for name in FOREIGN_PICTURES for mode, settings in FOREIGN_SETTINGS]
    return _made['foreign']


def foreign_reference(i):
    """``reference_decode`` of foreign stream i — made once."""
    if ('reference', i) not in _made:
        _made['reference', i] = reference_decode(foreign_streams()[i][1])
    return _made['reference', i]


# bit positions in the scan, one flipped bit each: found by a search over both scans for flips that leave every marker alone and end in each of the flags
# that damage to the bits can raise (SIZE needs a table that lists a symbol no baseline coder emits: test_a_hostile_table in the host tests)
FLIPS = {'own': (273, 1508, 2002, 3484, 3978, 4004, 5343), 'foreign': (0, 260, 780, 3263, 3432, 4212, 5512)}


def damaged_streams():
    """[(label, stream, the undamaged stream)] — 20 of them, the header intact: scans truncated inside an interval, single flipped bits at FLIPS on two
    streams (none makes or unmakes a marker, so the intervals stay), an interval replaced by 0xFF 0x00 pairs, a last interval without a byte."""
    if 'damaged' in _made:
        return _made['damaged']
    from pix2pix3d_amd import video
    own = video.encode_jpeg(torch.from_numpy(PICTURES['gradient'])[None], 90, '4:4:4')[0]
    foreign = pillow_jpeg(PICTURES['noise'], 'RGB', quality=90, subsampling=2, restart_marker_blocks=2, optimize=True)
    out = []

    def scan_range(stream):
        return len(stream) - 2 - len(split_jpeg(stream)[1]), len(stream) - 2

    def intact(stream, damaged):
        """No marker made or unmade: the 0xFF bytes and what follows them are where they were."""
        a, b = (np.frombuffer(s, dtype=np.uint8) for s in (stream, damaged))
        return len(a) == len(b) and np.array_equal(a == 0xFF, b == 0xFF) and np.array_equal(a[1:][a[:-1] == 0xFF], b[1:][b[:-1] == 0xFF])
    for label, stream in (('own', own), ('foreign', foreign)):
        begin, end = scan_range(stream)
        for at in FLIPS[label]:
            damaged = bytearray(stream)
            damaged[begin + (at >> 3)] ^= 0x80 >> (at & 7)
            assert intact(stream, bytes(damaged))
            out.append((f'{label}: bit {at} flipped', bytes(damaged), stream))
        # truncated inside the last interval: its tail is gone, EOI stays
        out.append((f'{label}: truncated', stream[:end - 9] + stream[end:], stream))
        # the second interval replaced by stuffed 0xFF bytes: all-ones bits
        marks = [i for i in range(begin, end - 1) if stream[i] == 0xFF and 0xD0 <= stream[i + 1] <= 0xD7]
        out.append((f'{label}: an interval of FF 00', stream[:marks[0] + 2] + b'\xff\x00' * 6 + stream[marks[1]:], stream))
    # and two truncations that cut deeper
    for label, stream in (('own', own), ('foreign', foreign)):
        begin, end = scan_range(stream)
        last = max(i for i in range(begin, end - 1) if stream[i] == 0xFF and 0xD0 <= stream[i + 1] <= 0xD7) + 2
        out.append((f'{label}: the last interval empty', stream[:last] + stream[end:], stream))
    assert len(out) == 20
    _made['damaged'] = out
    return out


# ---- the case file of tools/jpeg_unscan_check.cpp -------------------------------------------------------------------------------------------------
def unscan_arguments(stream):
    """The arguments of ``jpeg_unscan`` for ONE stream, from ``jpeg_parse``: (data, ranges, h, w, subsampling, tables, table_of_frame, restart, components)."""
    from pix2pix3d_amd import video
    info = video.jpeg_parse(stream)
    data = torch.tensor(list(stream[info.scan[0]:info.scan[1]]), dtype=torch.uint8)
    ranges = torch.from_numpy(info.intervals - info.scan[0])[None]
    tables = torch.stack([video.jpeg_decode_tables(*t) for t in info.huffman])[None]
    return data, ranges, info.h, info.w, info.subsampling, tables, torch.zeros([1], dtype=torch.int32), info.restart, info.components


def all_cases():
    """[(label, the arguments of ``jpeg_unscan``)] of everything the tests decode: the round trips, the foreign streams, the damaged ones."""
    from pix2pix3d_amd import video
    cases = []
    for name in ROUND_TRIPS:
        c = round_trip(name)
        n_intervals = video.jpeg_layout(c['h'], c['w'], c['subsampling'])[3]
        cases.append((name, (c['data'], own_ranges(c['data'], c['offsets'], n_intervals), c['h'], c['w'], c['subsampling'], None, None, video.JPEG_RESTART, 3)))
    cases += [(label, unscan_arguments(stream)) for label, stream, _ in foreign_streams()]
    cases += [(label, unscan_arguments(stream)) for label, stream, _ in damaged_streams()]
    return cases


def write_case_file(path, cases):
    from pix2pix3d_amd import video
    with open(path, 'wb') as fh:
        fh.write(b'JUC1' + struct.pack('<i', len(cases)))
        for _, (data, ranges, h, w, subsampling, tables, table_of_frame, restart, components) in cases:
            f = ranges.shape[0]
            if tables is None:
                tables = torch.stack([video.jpeg_decode_tables(*t) for t in zip(video.jpeg_huffman().bits, video.jpeg_huffman().values)])[None]
            if table_of_frame is None:
                table_of_frame = torch.zeros([f], dtype=torch.int32)
            n_mcu = video.jpeg_layout(h, w, subsampling)[1]
            fh.write(struct.pack('<7iq', h, w, 1 if subsampling == '4:2:0' else 0, components, restart or n_mcu, f, tables.shape[0], data.shape[0]))
            for t in (ranges, tables, table_of_frame, data):
                fh.write(t.contiguous().numpy().tobytes())


def read_results(path, cases):
    """[(coefficients, status)] as the stand-alone program wrote them."""
    from pix2pix3d_amd import video
    raw, at, out = open(path, 'rb').read(), 0, []
    for _, (data, ranges, h, w, subsampling, *_) in cases:
        _, n_mcu, bpm, _ = video.jpeg_layout(h, w, subsampling)
        f, n_intervals = ranges.shape[:2]
        n = f * n_mcu * bpm * 64
        coefficients = np.frombuffer(raw, dtype=np.int16, count=n, offset=at).reshape(f, n_mcu, bpm, 64)
        status = np.frombuffer(raw, dtype=np.int32, count=f * n_intervals, offset=at + 2 * n).reshape(f, n_intervals)
        at += 2 * n + 4 * f * n_intervals
        out.append((torch.from_numpy(coefficients.copy()), torch.from_numpy(status.copy())))
    assert at == len(raw)
    return out


def build_checker(directory, sanitize=True):
    """(path of the stand-alone decoder built from tools/jpeg_unscan_check.cpp, whether it carries the sanitizers).  A host compiler only: no HIP, no
    Python.  Where no compiler links the sanitizer runtimes, the plain build — and False."""
    from pix2pix3d_amd import build
    source, include = os.path.join(ROOT, 'tools', 'jpeg_unscan_check.cpp'), os.path.join(build.CSRC, 'video')
    compilers = [c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++')) if c]
    attempts = [(c, True) for c in compilers if sanitize] + [(c, False) for c in compilers]
    log = []
    for compiler, sanitized in attempts:
        exe = os.path.join(directory, 'jpeg_unscan_check' + ('_san' if sanitized else ''))
        flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-O1', '-g'] if sanitized else ['-O2']
        r = subprocess.run([compiler, '-std=c++17', '-Wall', *flags, '-I', include, source, '-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode == 0:
            return exe, sanitized
        log.append(f'{compiler} {" ".join(flags)}:\n{r.stdout}')
    raise AssertionError('no host compiler built tools/jpeg_unscan_check.cpp:\n' + '\n'.join(log))


def run_checker(exe, cases, directory):
    """The results of the stand-alone program on ``cases``; it must end with status 0 and nothing on stderr (a sanitizer report is both)."""
    case_file, result_file = os.path.join(directory, 'cases.bin'), os.path.join(directory, 'results.bin')
    write_case_file(case_file, cases)
    r = subprocess.run([exe, case_file, result_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == '', (r.returncode, r.stdout, r.stderr)
    return read_results(result_file, cases)
