"""Lossless frames, PNG and APNG, without PIL: every frame a zlib stream made where the frames are.

``encode_png`` runs three stages that csrc/video/p3d_video.h states in integers (``png_filter``: the PNG row filters; ``png_counts``: the symbol counts of
run-length deflate per segment; ``png_deflate``: one length-limited Huffman code a frame, made on the host between count and emit, and the bytes); what
does not touch pixels (chunks, CRC-32) is host work too.  ``save_png`` / ``save_png_sequence`` write stills, ``save_apng`` an animated PNG, and
``png_chunks`` takes a file apart again; 1 .. 4 bytes a pixel, palette indices and 16-bit grey (``depth16``) included."""
import numpy as np
import torch

from .. import _lib
from ..clips import HEADER, MAX_PIXELS, check, check_frames, clip_args, video_lib

COLORS = HEADER.constants['P3D_VIDEO_COLORS']        # the rows of a palette, as gif.py reads it
PNG_SYMBOLS, PNG_STATS, PNG_HEADER_WORDS, PNG_ADAPTIVE = (HEADER.constants['P3D_VIDEO_PNG_' + k] for k in ('SYMBOLS', 'STATS', 'HEADER_WORDS', 'ADAPTIVE'))
PNG_SEGMENT_BYTES = 32768                            # filtered bytes of a segment, about: the unit of parallel work (DESIGN.md section 2.1v records the choice)
PNG_MODES = {'L': (1, 0, 8), 'LA': (2, 4, 8), 'RGB': (3, 2, 8), 'RGBA': (4, 6, 8), 'P': (1, 3, 8), 'I;16': (2, 0, 16)}      # mode: bytes a pixel, colour type, depth
PNG_FILTERS = {'none': 0, 'sub': 1, 'up': 2, 'average': 3, 'paeth': 4, 'adaptive': PNG_ADAPTIVE}
PNG_MAX_MATCH = 258
_PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'
_ADLER = 65521
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)       # RFC 1951 section 3.2.7: the order of the code-length code's lengths
_LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)      # of the symbols 257 .. 285
_LENGTH_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)


def _length_tables():
    """(symbol, extra bits, extra value) of every match length 0 .. 258, from the RFC's table (entries below 3 are unused)."""
    symbol, bits, value = (np.zeros(PNG_MAX_MATCH + 1, dtype=np.int64) for _ in range(3))
    for length in range(3, PNG_MAX_MATCH + 1):
        i = max(j for j, base in enumerate(_LENGTH_BASE) if base <= length)
        symbol[length], bits[length], value[length] = 257 + i, _LENGTH_EXTRA[i], length - _LENGTH_BASE[i]
    return symbol, bits, value


_LEN_SYMBOL, _LEN_BITS, _LEN_VALUE = _length_tables()


def _check_filter(filter):
    if isinstance(filter, str) and filter in PNG_FILTERS:
        return PNG_FILTERS[filter]
    if isinstance(filter, bool) or isinstance(filter, str) or int(filter) != filter or not 0 <= int(filter) <= PNG_ADAPTIVE:
        raise ValueError(f"filter must be 0 .. {PNG_ADAPTIVE} or one of {', '.join(PNG_FILTERS)}, got {filter!r}")
    return int(filter)


def _bpp(frames):
    return frames.shape[3] if frames.ndim == 4 else 1


def _check_filtered(filtered, what):
    if not torch.is_tensor(filtered) or filtered.dtype != torch.uint8 or filtered.ndim != 3:
        raise ValueError(f'{what}: filtered must be a uint8 [F, H, 1 + W bpp] tensor (png_filter)')
    f, h, r = filtered.shape
    if f * h * r >= MAX_PIXELS:
        raise ValueError(f'{what}: {f} x {h} x {r} filtered bytes reach 2^31')
    return f, h, r


def _check_segment_rows(segment_rows):
    if isinstance(segment_rows, bool) or int(segment_rows) != segment_rows or int(segment_rows) < 1:
        raise ValueError(f'segment_rows must be an integer >= 1, got {segment_rows!r}')
    return int(segment_rows)


def png_segment_rows(w, bpp):
    """The rows of a segment for pictures ``w`` pixels of ``bpp`` bytes wide: max(1, PNG_SEGMENT_BYTES // (1 + w bpp))."""
    return max(1, PNG_SEGMENT_BYTES // (1 + int(w) * int(bpp)))


def _png_filter_numpy(x, bpp, filt):
    """uint8 [H, 1 + n] of ONE frame ``x`` int64 [H, n]: the header's filter rule, every candidate in full."""
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, bpp:], b[1:], c[1:, bpp:] = x[:, :-bpp], x[:-1], x[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    residuals = np.stack([(x - pred) & 255 for pred in (0, a, b, (a + b) >> 1, paeth)])
    if filt == PNG_ADAPTIVE:
        types = np.where(residuals < 128, residuals, 256 - residuals).sum(axis=2).argmin(axis=0)      # argmin: the first, so the lowest type on a tie
    else:
        types = np.full(x.shape[0], filt, dtype=np.int64)
    chosen = np.take_along_axis(residuals, types[None, :, None], axis=0)[0]
    return np.concatenate([types[:, None], chosen], axis=1).astype(np.uint8)


def png_filter(frames, filter='adaptive'):
    """uint8 [F, H, 1 + W bpp]: every row as its filter type and its residuals — the PNG specification's None, Sub, Up, Average and Paeth, the row above a
    frame's first being zeros.  Frames uint8 [F, H, W] (bpp 1) or [F, H, W, bpp] (bpp 2 .. 4) with contiguous pixels and any pitches; ``filter`` 0 .. 4 or
    its name forces a type, 'adaptive' (5) takes per row the type with the smallest sum of |residual as int8|, the lowest on a tie (libpng's heuristic).
    Device tensors: ONE ``p3d_video_png_filter`` launch; CPU tensors: the numpy formulation."""
    f, h, w = check_frames(frames, 'png_filter', (1, 2, 3, 4))
    bpp, filt = _bpp(frames), _check_filter(filter)
    if f * h * (1 + w * bpp) >= MAX_PIXELS:
        raise ValueError(f'png_filter: {f} x {h} rows of {1 + w * bpp} filtered bytes reach 2^31')
    if f * h * w == 0:
        return torch.zeros([f, h, 1 + w * bpp], dtype=torch.uint8, device=frames.device)
    if not frames.is_cuda:
        return torch.from_numpy(np.stack([_png_filter_numpy(x.reshape(h, w * bpp).to(torch.int64).numpy(), bpp, filt) for x in frames]))
    out = torch.empty([f, h, 1 + w * bpp], dtype=torch.uint8, device=frames.device)
    with _lib.kernel_timer('video_png_filter', out):
        code = video_lib().p3d_video_png_filter(*clip_args(frames), bpp, filt, _lib.ptr(out), _lib.stream_of(out))
    check(code, 'video_png_filter')
    return out


def _png_tokens(b, segment_bytes):
    """(literals, match) per byte of ONE frame's filtered bytes ``b`` int64 [n], cut into segments of ``segment_bytes``: how many literals of itself the byte
    carries (0, 1, 2) and the length of the match that ends with it (0: none) — the header's token rule by position."""
    i = np.arange(b.shape[0])
    start = i % segment_bytes == 0
    start[1:] |= b[1:] != b[:-1]
    last = np.append(start[1:], True)
    k = i - np.maximum.accumulate(np.where(start, i, 0))                          # the byte's place in its run
    r = k % PNG_MAX_MATCH
    match = np.where((k > 0) & (r == 0), PNG_MAX_MATCH, np.where((k > 0) & last & (r >= 3), r, 0))
    literals = np.where(k == 0, 1, np.where(last & (r > 0) & (r < 3), r, 0))
    return literals, match


def _png_counts_numpy(b, segment_bytes):
    """int64 [S, PNG_STATS] of one frame's filtered bytes."""
    n = b.shape[0]
    n_seg = -(-n // segment_bytes)
    literals, match = _png_tokens(b, segment_bytes)
    i = np.arange(n)
    seg, on = i // segment_bytes, match > 0
    stats = np.bincount(seg * PNG_STATS + b, weights=literals, minlength=n_seg * PNG_STATS)
    stats += np.bincount(seg[on] * PNG_STATS + _LEN_SYMBOL[match[on]], minlength=n_seg * PNG_STATS)
    stats = stats.astype(np.int64).reshape(n_seg, PNG_STATS)
    stats[:, PNG_SYMBOLS] = np.bincount(seg[on], weights=_LEN_BITS[match[on]], minlength=n_seg)
    stats[:, PNG_SYMBOLS + 1] = np.bincount(seg[on], minlength=n_seg)
    firsts = np.arange(0, n, segment_bytes)
    sizes = np.minimum(segment_bytes, n - firsts)
    stats[:, PNG_SYMBOLS + 2] = np.add.reduceat(b, firsts) % _ADLER
    stats[:, PNG_SYMBOLS + 3] = np.add.reduceat(((sizes[seg] - i % segment_bytes) % _ADLER) * b, firsts) % _ADLER
    return stats


def png_counts(filtered, segment_rows):
    """int32 [F, S, PNG_STATS], S = ceil(H / segment_rows): per segment of ``segment_rows`` filtered rows the number of times every literal/length symbol is
    coded ([256], end of block, stays 0: it comes once a segment), at [286] the matches' extra bits, at [287] the matches, at [288:290] the Adler pair
    (s1 = sum b, s2 = sum (L - i) b_i, mod 65521).  The token rule is p3d_video.h's: runs of equal bytes, a literal, then matches at distance 1 of up to
    258.  Device tensors: ONE ``p3d_video_png_count`` launch, no synchronisation; CPU tensors: the numpy formulation."""
    f, h, r = _check_filtered(filtered, 'png_counts')
    rows = min(_check_segment_rows(segment_rows), max(h, 1))
    n_seg = -(-h // rows)
    if f * h == 0 or r <= 1:
        return torch.zeros([f, n_seg, PNG_STATS], dtype=torch.int32, device=filtered.device)
    filtered = filtered.contiguous()
    if not filtered.is_cuda:
        return torch.from_numpy(np.stack([_png_counts_numpy(x.reshape(-1).to(torch.int64).numpy(), rows * r) for x in filtered]).astype(np.int32))
    stats = torch.empty([f, n_seg, PNG_STATS], dtype=torch.int32, device=filtered.device)
    with _lib.kernel_timer('video_png_count', stats):
        code = video_lib().p3d_video_png_count(_lib.ptr(filtered), f, h, r, rows, _lib.ptr(stats), _lib.stream_of(stats))
    check(code, 'video_png_count')
    return stats


def png_code_lengths(counts, limit=15):
    """int64 [n]: the code length of every symbol of the histogram ``counts`` [n] (0 for an unused one) — an optimal prefix code among those of at most
    ``limit`` bits, by package-merge.  The used symbols are ordered by (count, symbol); ``limit`` times, the list of the level below is paired up into
    packages and merged with the symbols by weight, a symbol before a package of its weight; the lightest 2 u - 2 items of the top list are taken (u used
    symbols), and a symbol's length is the number of levels at which it is taken — at every level a prefix of the ordered symbols, so only their number is
    tracked.  One used symbol gets one bit, none gets nothing.  ValueError when 2^limit codes are too few."""
    counts = np.asarray(torch.as_tensor(counts).cpu() if torch.is_tensor(counts) else counts, dtype=np.int64).reshape(-1)
    if (counts < 0).any():
        raise ValueError('png_code_lengths: counts must be >= 0')
    lengths = np.zeros(counts.shape[0], dtype=np.int64)
    order = np.flatnonzero(counts)
    order = order[np.argsort(counts[order], kind='stable')]                       # by (count, symbol)
    u = order.shape[0]
    if u > 1 << int(limit):
        raise ValueError(f'png_code_lengths: {u} symbols do not fit {limit} bits')
    if u <= 1:
        lengths[order] = 1
        return lengths
    weights = counts[order]
    is_symbol = np.ones(u, dtype=bool)
    level_w, levels = weights, [is_symbol]
    for _ in range(int(limit) - 1):
        pairs = level_w.shape[0] // 2
        both = np.concatenate([weights, level_w[0:2 * pairs:2] + level_w[1:2 * pairs:2]])
        by_weight = np.argsort(both, kind='stable')                               # the symbols stand first: they win ties
        level_w = both[by_weight]
        levels.append(by_weight < u)
    need, by_rank = 2 * u - 2, np.zeros(u, dtype=np.int64)
    for symbols in reversed(levels):
        taken = int(symbols[:need].sum())
        by_rank[:taken] += 1
        need = 2 * (min(need, symbols.shape[0]) - taken)
    lengths[order] = by_rank
    return lengths


def png_canonical_codes(lengths):
    """int64 [n]: the canonical code of every symbol as RFC 1951 section 3.2.2 assigns it from the code ``lengths`` — codes of one length count up in symbol
    order, the first of a length is (the first of the length before + their number) << 1.  A symbol of length 0 has no code (0)."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    per_length = np.bincount(lengths, minlength=2)
    per_length[0] = 0
    codes, code = np.zeros_like(lengths), 0
    for bits in range(1, per_length.shape[0]):
        code = (code + int(per_length[bits - 1])) << 1
        of_length = np.flatnonzero(lengths == bits)
        codes[of_length] = code + np.arange(of_length.shape[0])
    return codes


def _reversed(codes, lengths):
    """Every code with its ``lengths`` bits in reverse order: what a deflate stream, packed from the low bit on, takes."""
    codes, out = np.asarray(codes, dtype=np.int64), np.zeros_like(np.asarray(codes, dtype=np.int64))
    for bit in range(int(np.max(lengths, initial=0))):
        out |= np.where(lengths > bit, ((codes >> bit) & 1) << (lengths - 1 - bit).clip(min=0), 0)
    return out


def png_block_header(lengths):
    """``(bits, n)``: the header of a dynamic-Huffman deflate block for the literal/length code ``lengths`` [286] and the constant distance code (symbols 0 and
    1, one bit each), WITHOUT its BFINAL bit, as an int whose bit i is the i-th bit of the stream, and their number.  BTYPE = 10; HLIT = (the last used symbol
    + 1, at least 257) - 257; HDIST = 1; the lengths of both codes in one sequence, run-length coded by this greedy rule, from the front: a run of zeros of
    11 or more gives 18 with up to 138 of them, of 3 .. 10 gives 17, a shorter one a plain 0; any other length is written once and, while 3 or more equal
    ones follow, 16 with up to 6 of them.  The code-length code over what that used is ``png_code_lengths`` at a limit of 7 bits (a lone symbol gets a
    partner of length 1, so the code is complete), HCLEN trims the unused tail of its fixed order."""
    lengths = [int(v) for v in np.asarray(lengths).reshape(-1)]
    if len(lengths) != PNG_SYMBOLS or not all(0 <= v <= 15 for v in lengths):
        raise ValueError(f'png_block_header: lengths must be {PNG_SYMBOLS} values 0 .. 15')
    n_lit = max(257, max((s + 1 for s, v in enumerate(lengths) if v), default=0))
    sequence = lengths[:n_lit] + [1, 1]
    symbols, i = [], 0                                                            # (symbol, extra bits, extra value)
    while i < len(sequence):
        v, run = sequence[i], 1
        while i + run < len(sequence) and sequence[i + run] == v:
            run += 1
        if v == 0 and run >= 11:
            take = min(run, 138)
            symbols.append((18, 7, take - 11))
        elif v == 0 and run >= 3:
            take = run
            symbols.append((17, 3, take - 3))
        else:
            take = 1
            symbols.append((v, 0, 0))
            while v and run - take >= 3:
                more = min(run - take, 6)
                symbols.append((16, 2, more - 3))
                take += more
        i += take
    used = np.bincount([s for s, _, _ in symbols], minlength=19)
    cl_lengths = png_code_lengths(used, limit=7)
    if (used > 0).sum() == 1:
        cl_lengths[0 if used[0] == 0 else 18] = 1
    cl_codes = _reversed(png_canonical_codes(cl_lengths), cl_lengths)
    n_cl = max(4, max(j + 1 for j, s in enumerate(_CL_ORDER) if cl_lengths[s]))
    bits, n = 0, 0

    def put(value, count):
        nonlocal bits, n
        bits |= int(value) << n
        n += int(count)
    put(2, 2)
    put(n_lit - 257, 5)
    put(1, 5)
    put(n_cl - 4, 4)
    for s in _CL_ORDER[:n_cl]:
        put(cl_lengths[s], 3)
    for s, extra_bits, extra in symbols:
        put(cl_codes[s], cl_lengths[s])
        put(extra, extra_bits)
    return bits, n


class _PngPlan:
    """What the host makes of ONE frame's counts ``stats`` int64 [S, PNG_STATS] and the bytes of its segments ``sizes`` [S]: the code, the block header, the
    bytes every segment takes, and the frame's Adler-32."""

    def __init__(self, stats, sizes):
        n_seg = stats.shape[0]
        counts = stats[:, :PNG_SYMBOLS].sum(axis=0)
        counts[256] = n_seg
        self.lengths = png_code_lengths(counts, 15)
        self.codes = _reversed(png_canonical_codes(self.lengths), self.lengths)
        self.table = (self.lengths << 16 | self.codes).astype(np.uint32)
        self.header, self.header_bits = png_block_header(self.lengths)
        bits = 1 + self.header_bits + stats[:, :PNG_SYMBOLS] @ self.lengths + stats[:, PNG_SYMBOLS] + stats[:, PNG_SYMBOLS + 1] + self.lengths[256]
        self.segment_bytes = (bits + 3 + 7) // 8 + 4                                # the empty stored block after it
        self.segment_bytes[-1] = (bits[-1] + 7) // 8
        s1, s2 = 1, 0
        for size, a, b in zip(sizes.tolist(), stats[:, PNG_SYMBOLS + 2].tolist(), stats[:, PNG_SYMBOLS + 3].tolist()):
            s2 = (s2 + size * s1 + b) % _ADLER
            s1 = (s1 + a) % _ADLER
        self.adler = s2 << 16 | s1

    def header_words(self):
        return np.frombuffer(self.header.to_bytes(4 * PNG_HEADER_WORDS, 'little'), dtype=np.uint32)


def _png_segment_numpy(b, literals, match, plan, final, n_bytes):
    """The bytes of ONE segment: its filtered bytes ``b`` int64 and their tokens."""
    lengths, codes = plan.lengths, plan.codes
    value = np.where(literals == 2, codes[b] | codes[b] << lengths[b], np.where(literals == 1, codes[b], 0))
    count = literals * lengths[b]
    on = match > 0
    symbol = _LEN_SYMBOL[match[on]]
    value[on] = codes[symbol] | _LEN_VALUE[match[on]] << lengths[symbol]            # and the distance code, a 0 bit
    count[on] = lengths[symbol] + _LEN_BITS[match[on]] + 1
    bits = np.zeros(8 * n_bytes, dtype=np.uint8)
    bits[0] = final
    bits[1:1 + plan.header_bits] = [(plan.header >> i) & 1 for i in range(plan.header_bits)]
    first = 1 + plan.header_bits + np.cumsum(count) - count
    for bit in range(int(count.max(initial=0))):
        has = count > bit
        bits[first[has] + bit] = (value[has] >> bit) & 1
    at = 1 + plan.header_bits + int(count.sum())
    bits[at:at + lengths[256]] = [(int(codes[256]) >> i) & 1 for i in range(lengths[256])]
    if not final:
        bits[-16:] = 1                                                              # 00 00 FF FF
    return np.packbits(bits, bitorder='little')


def _png_segment_sizes(h, r, rows):
    firsts = np.arange(0, h, rows)
    return np.minimum(rows, h - firsts) * r


def png_deflate(filtered, segment_rows):
    """``(data uint8 [total], offsets int64 [F + 1])``: the zlib stream of every frame of ``filtered`` (``png_filter``'s rows), frame i at
    ``data[offsets[i]:offsets[i + 1]]``; ``data`` on the filtered bytes' device, ``offsets`` on the host.  78 01, then the frame's segments of ``segment_rows``
    rows, each a dynamic-Huffman block of its own under the frame's ONE code (all but the last followed by an empty stored block, so that every segment starts
    on a byte), then the Adler-32.  Device tensors: ``p3d_video_png_count``, the copy of the counts to the host — the ONLY synchronisation —, there one code, one
    block header and the exact byte length of every segment a frame, their upload in one pinned buffer, and ``p3d_video_png_emit``.  CPU tensors: the numpy
    formulation.  No pixel (F H = 0, or rows of the type byte only): no stream, ``offsets`` all 0."""
    return _png_deflate(filtered, segment_rows)[:2]


def _png_deflate(filtered, segment_rows):
    """``png_deflate`` and, third, int64 numpy [F, S]: the bytes every segment takes in its frame's stream (what the segment index is made from)."""
    f, h, r = _check_filtered(filtered, 'png_deflate')
    rows = min(_check_segment_rows(segment_rows), max(h, 1))
    if f * h == 0 or r <= 1:
        return torch.zeros([0], dtype=torch.uint8, device=filtered.device), torch.zeros([f + 1], dtype=torch.int64), np.zeros([f, 0], dtype=np.int64)
    filtered = filtered.contiguous()
    stats = png_counts(filtered, rows)
    host = stats.cpu().numpy().astype(np.int64)
    sizes = _png_segment_sizes(h, r, rows)
    n_seg = sizes.shape[0]
    plans = [_PngPlan(s, sizes) for s in host]
    lengths = np.stack([p.segment_bytes for p in plans])                            # [F, S]
    frame_bytes = lengths.sum(axis=1) + 6
    offsets = np.concatenate([[0], np.cumsum(frame_bytes)])
    starts = offsets[:-1, None] + 2 + np.cumsum(lengths, axis=1) - lengths
    if not filtered.is_cuda:
        out = np.zeros(int(offsets[-1]), dtype=np.uint8)
        for i, plan in enumerate(plans):
            b = filtered[i].reshape(-1).to(torch.int64).numpy()
            literals, match = _png_tokens(b, rows * r)
            out[offsets[i]:offsets[i] + 2] = (0x78, 0x01)
            for s in range(n_seg):
                part = slice(s * rows * r, s * rows * r + int(sizes[s]))
                out[starts[i, s]:starts[i, s] + lengths[i, s]] = _png_segment_numpy(b[part], literals[part], match[part], plan, s == n_seg - 1, int(lengths[i, s]))
            out[offsets[i + 1] - 4:offsets[i + 1]] = list(plan.adler.to_bytes(4, 'big'))
        return torch.from_numpy(out), torch.from_numpy(offsets.astype(np.int64)), lengths
    parts = [starts.astype(np.int64).reshape(-1), np.stack([p.table for p in plans]).reshape(-1), np.concatenate([p.header_words() for p in plans]),
             np.array([p.header_bits for p in plans], dtype=np.int32), np.array([p.adler for p in plans], dtype=np.uint32)]
    at = np.concatenate([[0], np.cumsum([p.nbytes for p in parts])])                 # the int64 part first: every part stays aligned
    pinned = torch.empty([int(at[-1])], dtype=torch.uint8, pin_memory=True)
    pinned.numpy()[:] = np.concatenate([p.view(np.uint8) for p in parts])
    up = torch.empty([int(at[-1])], dtype=torch.uint8, device=filtered.device)
    up.copy_(pinned, non_blocking=True)                                             # (pinned, so the copy does not wait for the device)
    data = torch.empty([int(offsets[-1])], dtype=torch.uint8, device=filtered.device)
    import ctypes
    where = [ctypes.c_void_p(up.data_ptr() + int(a)) for a in at[:-1]]
    with _lib.kernel_timer('video_png_emit', data):
        code = video_lib().p3d_video_png_emit(_lib.ptr(filtered), f, h, r, rows, where[1], where[2], where[3], where[4], where[0], _lib.ptr(data), data.shape[0],
                                              _lib.stream_of(data))
    check(code, 'video_png_emit')
    return data, torch.from_numpy(offsets.astype(np.int64)), lengths


def _png_chunk(kind, payload):
    import zlib
    return len(payload).to_bytes(4, 'big') + kind + payload + zlib.crc32(kind + payload).to_bytes(4, 'big')


def _palette_bytes(palette):
    pal = torch.as_tensor(palette).detach().cpu()
    if pal.dtype != torch.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= COLORS:
        raise ValueError(f"mode 'P' needs a palette uint8 [n, 3] with 1 <= n <= {COLORS}")
    return pal.contiguous().numpy().tobytes()


def png_header(h, w, mode, palette=None):
    """Everything of a PNG file before its image data: the signature, IHDR (``w``, ``h``, the depth and colour type of ``mode`` — ``PNG_MODES`` —, deflate,
    adaptive filtering, no interlace) and, for mode 'P', PLTE from ``palette`` uint8 [n <= 256, 3]."""
    if mode not in PNG_MODES:
        raise ValueError(f'mode must be one of {", ".join(PNG_MODES)}, got {mode!r}')
    if not (1 <= int(h) < 1 << 31 and 1 <= int(w) < 1 << 31):
        raise ValueError(f'a PNG is 1 .. 2^31 - 1 pixels a side, got {h} x {w}')
    if (mode == 'P') != (palette is not None):
        raise ValueError("a palette goes with mode 'P', and only with it")
    _, colour_type, depth = PNG_MODES[mode]
    out = _PNG_SIGNATURE + _png_chunk(b'IHDR', int(w).to_bytes(4, 'big') + int(h).to_bytes(4, 'big') + bytes([depth, colour_type, 0, 0, 0]))
    return out + (_png_chunk(b'PLTE', _palette_bytes(palette)) if mode == 'P' else b'')


def _segment_index(segment_rows, lengths):
    """The seGM chunk of ONE frame whose segments take ``lengths`` bytes: big-endian uint32 ``segment_rows``, then for every segment but the first the offset
    of its first byte in the frame's zlib stream.  An ancillary, private, unsafe-to-copy chunk: a reader that does not know it skips it, an editor drops it."""
    firsts = 2 + np.cumsum(lengths)[:-1]
    return _png_chunk(b'seGM', b''.join(int(v).to_bytes(4, 'big') for v in [segment_rows, *firsts.tolist()]))


def _png_streams(frames, mode, palette, filter, what, index=False):
    """(frames' F, H, W, the mode, the zlib stream of every frame as bytes, the seGM chunk of every frame: empty without ``index``)."""
    frames = torch.as_tensor(frames)
    if mode is None:
        if not torch.is_tensor(frames) or frames.ndim not in (3, 4) or (frames.ndim == 4 and frames.shape[3] not in (2, 3, 4)):
            raise ValueError(f'{what}: frames must be uint8 [F, H, W] or [F, H, W, 2 .. 4]')
        mode = 'L' if frames.ndim == 3 else {2: 'LA', 3: 'RGB', 4: 'RGBA'}[frames.shape[3]]
    if mode not in PNG_MODES:
        raise ValueError(f'{what}: mode must be one of {", ".join(PNG_MODES)}, got {mode!r}')
    bpp = PNG_MODES[mode][0]
    f, h, w = check_frames(frames, what, (bpp,))
    if (mode == 'P') != (palette is not None):
        raise ValueError(f"{what}: a palette goes with mode 'P', and only with it")
    if f and (h == 0 or w == 0):
        raise ValueError(f'{what}: a PNG has at least one pixel, got {h} x {w}')
    if f == 0:
        return (f, h, w), mode, [], []
    filtered = png_filter(frames, (0 if mode == 'P' else PNG_ADAPTIVE) if filter is None else filter)
    rows = png_segment_rows(w, bpp)
    data, offsets, lengths = _png_deflate(filtered, rows)
    data, offsets = data.cpu().numpy().tobytes(), offsets.tolist()
    return (f, h, w), mode, [data[offsets[i]:offsets[i + 1]] for i in range(f)], [_segment_index(rows, lengths[i]) if index else b'' for i in range(f)]


def encode_png(frames, mode=None, palette=None, filter=None, index=False):
    """A list of ``bytes``, one complete PNG file per frame: ``png_header``, one IDAT with the frame's zlib stream, IEND.  Frames uint8, on the device or the host
    (or a numpy array), read in place whatever their pitches: [F, H, W] is 'L', [F, H, W, 2] 'LA', [F, H, W, 3] 'RGB', [F, H, W, 4] 'RGBA' when ``mode`` is None;
    ``mode='P'`` takes [F, H, W] indices with ``palette`` uint8 [n <= 256, 3] (every index below n: not checked, it would take a synchronisation), and
    ``mode='I;16'`` takes [F, H, W, 2] big-endian byte pairs (``depth16``).  ``filter``: see ``png_filter``; None is 'none' for 'P', as the specification
    recommends, and 'adaptive' otherwise.  Lossless: a decoder returns the frames' bytes.  From device frames: three launches (filter, count, emit), ONE
    synchronisation with the host (the segments' counts come down, one code a frame goes up) and ONE device -> host copy, of the compressed bytes.  The
    chunks' CRC-32 is ``zlib.crc32`` on the host over those bytes.  ``index=True`` writes the segment index, a private ancillary chunk seGM before the
    frame's data: ``png_read.decode_png`` then inflates every segment as a part of its own (a 512 x 512 RGB picture: 24 lanes, not one); any other
    reader skips the chunk.  The default writes the bytes it always wrote."""
    (f, h, w), mode, streams, indices = _png_streams(frames, mode, palette, filter, 'encode_png', index)
    if not streams:
        return []
    header, end = png_header(h, w, mode, palette), _png_chunk(b'IEND', b'')
    return [header + segments + _png_chunk(b'IDAT', s) + end for s, segments in zip(streams, indices)]


def save_png(path, frame, mode=None, palette=None, filter=None, index=False):
    """One frame — uint8 [H, W] or [H, W, bpp], on the device or the host — as a PNG file (``encode_png``).  Returns its bytes."""
    frame = torch.as_tensor(frame)
    if frame.ndim not in (2, 3):
        raise ValueError(f'save_png: frame must be uint8 [H, W] or [H, W, bpp], got {tuple(frame.shape)}')
    stream, = encode_png(frame[None], mode, palette, filter, index)
    with open(path, 'wb') as fh:
        fh.write(stream)
    return stream


def save_png_sequence(pattern, frames, mode=None, palette=None, filter=None, index=False):
    """Every frame as a PNG file of its own, frame i at ``pattern.format(i)`` (say 'frame_{:04d}.png'), all encoded in one pass of ``encode_png``.  Returns
    the paths."""
    paths = []
    for i, stream in enumerate(encode_png(frames, mode, palette, filter, index)):
        paths.append(str(pattern).format(i))
        with open(paths[-1], 'wb') as fh:
            fh.write(stream)
    return paths


def save_apng(path, frames, fps=60, loops=0, mode=None, palette=None, filter=None, index=False):
    """The frames (``encode_png``'s contract) as an animated PNG: IHDR (and PLTE), acTL (the number of frames; ``loops`` plays, 0 for ever), then per frame fcTL —
    the whole canvas, the delay 1 / ``fps`` as a fraction of 16-bit terms, dispose 0 (none), blend 0 (source) — and its zlib stream, as IDAT for frame 0 (a
    viewer without APNG shows it) and as fdAT after that, fcTL and fdAT sharing one running sequence number.  Every frame is coded whole: bit-exact and
    independent of its neighbours.  ValueError for no frame.  Returns the zlib streams."""
    import fractions
    rate = fractions.Fraction(fps)
    if rate <= 0:
        raise ValueError(f'save_apng: fps must be > 0, got {fps!r}')
    delay = (1 / rate).limit_denominator(65535)
    if delay.numerator > 65535:
        raise ValueError(f'save_apng: a frame of {float(1 / rate)} s does not fit the 16-bit delay')
    if isinstance(loops, bool) or int(loops) != loops or not 0 <= int(loops) < 1 << 31:
        raise ValueError(f'save_apng: loops must be an integer >= 0, got {loops!r}')
    (f, h, w), mode, streams, indices = _png_streams(frames, mode, palette, filter, 'save_apng', index)
    if f == 0:
        raise ValueError('save_apng: an APNG needs at least one frame')
    out, sequence = [png_header(h, w, mode, palette), _png_chunk(b'acTL', f.to_bytes(4, 'big') + int(loops).to_bytes(4, 'big'))], 0
    for i, s in enumerate(streams):
        control = w.to_bytes(4, 'big') + h.to_bytes(4, 'big') + bytes(8) + delay.numerator.to_bytes(2, 'big') + delay.denominator.to_bytes(2, 'big') + bytes(2)
        out.append(_png_chunk(b'fcTL', sequence.to_bytes(4, 'big') + control))
        sequence += 1
        out.append(indices[i])                                                      # (seGM, or nothing: it describes the data chunk that follows)
        if i == 0:
            out.append(_png_chunk(b'IDAT', s))
        else:
            out.append(_png_chunk(b'fdAT', sequence.to_bytes(4, 'big') + s))
            sequence += 1
    out.append(_png_chunk(b'IEND', b''))
    with open(path, 'wb') as fh:
        fh.write(b''.join(out))
    return streams


def png_chunks(data):
    """``[(type, payload)]`` of a PNG or APNG file's bytes (or of the file at a path), in order — for tests, and for users without a viewer.  ValueError for a
    wrong signature, a chunk that runs past the end, a CRC-32 that does not match, or bytes after IEND."""
    import zlib
    if not isinstance(data, (bytes, bytearray)):
        with open(data, 'rb') as fh:
            data = fh.read()
    if data[:8] != _PNG_SIGNATURE:
        raise ValueError('png_chunks: not a PNG signature')
    at, chunks = 8, []
    while at < len(data):
        size, kind = int.from_bytes(data[at:at + 4], 'big'), bytes(data[at + 4:at + 8])
        if at + 12 + size > len(data):
            raise ValueError(f'png_chunks: the chunk {kind!r} at {at} runs past the end')
        payload = bytes(data[at + 8:at + 8 + size])
        if zlib.crc32(kind + payload) != int.from_bytes(data[at + 8 + size:at + 12 + size], 'big'):
            raise ValueError(f'png_chunks: the CRC of the chunk {kind!r} at {at} does not match')
        chunks.append((kind, payload))
        at += 12 + size
        if kind == b'IEND' and at != len(data):
            raise ValueError(f'png_chunks: {len(data) - at} bytes after IEND')
    if not chunks or chunks[0][0] != b'IHDR' or chunks[-1][0] != b'IEND':
        raise ValueError('png_chunks: a PNG runs from IHDR to IEND')
    return chunks


def depth16(depth, lo, hi):
    """uint8 [..., 2]: float ``depth`` as the big-endian byte pairs of 16-bit samples, mode 'I;16' of ``encode_png`` — clamp(floor((d - lo) / (hi - lo) 65535 +
    0.5), 0, 65535) in fp64 torch ops on the depth's device; no kernel of this package, no synchronisation.  NaN becomes 0."""
    depth = torch.as_tensor(depth)
    if not float(hi) > float(lo):
        raise ValueError(f'depth16: hi must be above lo, got {lo!r} .. {hi!r}')
    v = torch.floor((depth.to(torch.float64) - float(lo)) / (float(hi) - float(lo)) * 65535 + 0.5)
    v = torch.nan_to_num(v, nan=0.0).clamp(0, 65535).to(torch.int64)
    return torch.stack([v >> 8, v & 255], dim=-1).to(torch.uint8)


# The two launches of the way back (png_read.py), beside the other calls into the library: every entry point of the PNG stages is
# called from this module.
def _inflate_launch(data, parts, out, status):
    """``p3d_video_png_inflate`` on device tensors: the fill of ``out`` and a lane per row of ``parts``; no synchronisation."""
    with _lib.kernel_timer('video_png_inflate', out):
        code = video_lib().p3d_video_png_inflate(_lib.ptr(data), data.shape[0], _lib.ptr(parts), parts.shape[0], _lib.ptr(out), out.shape[0], _lib.ptr(status),
                                                 _lib.stream_of(out))
    check(code, 'video_png_inflate')


def _unfilter_launch(filtered, bpp, frames, status):
    """``p3d_video_png_unfilter`` on device tensors: ``filtered`` [F, H, 1 + W bpp] contiguous into the clip ``frames``, whatever its pitches."""
    f, h, r = filtered.shape
    with _lib.kernel_timer('video_png_unfilter', frames):
        code = video_lib().p3d_video_png_unfilter(_lib.ptr(filtered), f, h, (r - 1) // bpp, bpp, _lib.ptr(frames), frames.stride(0), frames.stride(1),
                                                  _lib.ptr(status), _lib.stream_of(frames))
    check(code, 'video_png_unfilter')
