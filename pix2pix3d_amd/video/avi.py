"""Motion-JPEG AVI: the clip as a RIFF file of ``jpeg.encode_jpeg``'s streams, which needs no codec library to write and which ffmpeg, VLC and OpenCV read.

``save_avi`` writes one, ``read_avi`` takes one apart again on the host, ``decode_avi`` shows it as its viewers see it (``jpeg_read.decode_jpeg``), and
``check_avi`` says whether a file shows what ``jpeg.jpeg_reconstruct`` promised (DESIGN.md sections 2.1u, 2.1x and 2.1y)."""
import torch

from .. import quality as Q
from ..clips import check_frames
from .jpeg import encode_jpeg, jpeg_reconstruct
from .jpeg_read import decode_jpeg

MAX_AVI_BYTES = 1 << 31                              # a RIFF file of one 'movi' list stays below it (OpenDML is out of scope)


def _chunk(fourcc, payload):
    return fourcc + len(payload).to_bytes(4, 'little') + payload + b'\0' * (len(payload) & 1)


def save_avi(path, frames, fps=60, quality=90, subsampling='4:2:0', psnr=None, ssim=None, ms_ssim=None):
    """The frames (``encode_jpeg``'s contract) as a Motion-JPEG AVI: a RIFF 'AVI ' file with the list 'hdrl' ('avih', and one 'strl' of 'strh' — 'vids' /
    'MJPG', the rate ``fps`` as dwRate / dwScale — and 'strf', a 40-byte BITMAPINFOHEADER of 24 bits), the list 'movi' of one '00dc' chunk per frame,
    padded to an even length, and 'idx1': per frame the key-frame flag, the chunk's offset from 'movi' and its length.  Every frame is a key frame.
    ValueError for no frame and for a file that would reach 2^31 bytes (OpenDML is out of scope).  ``psnr`` / ``ssim`` / ``ms_ssim``:
    ``encode_jpeg``'s target, which then picks the quality.  Returns the JPEG streams."""
    import fractions
    import struct
    frames = torch.as_tensor(frames)
    f, h, w = check_frames(frames)
    if f == 0:
        raise ValueError('save_avi: an AVI needs at least one frame')
    rate = fractions.Fraction(fps).limit_denominator(1 << 16)
    if rate <= 0:
        raise ValueError(f'save_avi: fps must be > 0, got {fps!r}')
    streams = encode_jpeg(frames, quality, subsampling, psnr, ssim, ms_ssim)
    movi, index = b'movi', b''
    chunks = [movi]
    at = 4                                                                        # of the next chunk, from the 'movi' word
    for s in streams:
        index += b'00dc' + struct.pack('<III', 0x10, at, len(s))                  # AVIIF_KEYFRAME
        chunks.append(_chunk(b'00dc', s))
        at += len(chunks[-1])
    largest = max(len(s) for s in streams)
    avih = struct.pack('<14I', round(1e6 / rate), int(largest * rate) + 1, 0, 0x10, f, 0, 1, largest, w, h, 0, 0, 0, 0)       # AVIF_HASINDEX
    strh = b'vidsMJPG' + struct.pack('<IHHIIIIIIIi4H', 0, 0, 0, 0, rate.denominator, rate.numerator, 0, f, largest, 0xFFFFFFFF, 0, 0, 0, w, h)
    strf = struct.pack('<IiiHH4sIiiII', 40, w, h, 1, 24, b'MJPG', 3 * w * h, 0, 0, 0, 0)
    hdrl = b'hdrl' + _chunk(b'avih', avih) + _chunk(b'LIST', b'strl' + _chunk(b'strh', strh) + _chunk(b'strf', strf))
    body = b'AVI ' + _chunk(b'LIST', hdrl) + _chunk(b'LIST', b''.join(chunks)) + _chunk(b'idx1', index)
    if len(body) + 8 >= MAX_AVI_BYTES:
        raise ValueError(f'save_avi: the file would take {len(body) + 8} bytes; an AVI of one RIFF chunk stays below 2^31')
    with open(path, 'wb') as fh:
        fh.write(b'RIFF' + len(body).to_bytes(4, 'little') + body)
    return streams


def read_avi(path):
    """``(the JPEG bytes of every frame, fps, (w, h))`` of a Motion-JPEG AVI, by following 'idx1' into 'movi' — for tests, and for users without a player.
    ``fps`` is dwRate / dwScale of the stream header, an int where that is whole.  ValueError for anything that is not such a file."""
    import struct
    with open(path, 'rb') as fh:
        data = fh.read()
    if len(data) < 12 or data[:4] != b'RIFF' or data[8:12] != b'AVI ':
        raise ValueError(f'read_avi: {path} is not a RIFF AVI file')

    def chunks(begin, end):
        """(fourcc, payload begin, payload end) of the chunks in data[begin:end]; of a LIST the fourcc is its type and the payload what follows it."""
        while begin + 8 <= end:
            fourcc, size = data[begin:begin + 4], int.from_bytes(data[begin + 4:begin + 8], 'little')
            if begin + 8 + size > end:
                raise ValueError(f'read_avi: the chunk {fourcc!r} at {begin} runs past its parent')
            yield (data[begin + 8:begin + 12], begin + 12, begin + 8 + size) if fourcc == b'LIST' else (fourcc, begin + 8, begin + 8 + size)
            begin += 8 + size + (size & 1)
    top = {name: (a, b) for name, a, b in chunks(12, min(len(data), 8 + int.from_bytes(data[4:8], 'little')))}
    if not all(name in top for name in (b'hdrl', b'movi', b'idx1')):
        raise ValueError(f'read_avi: {path} lacks one of hdrl, movi, idx1')
    strl = {name: (a, b) for name, a, b in chunks(*dict((n, (a, b)) for n, a, b in chunks(*top[b'hdrl']))[b'strl'])}
    strh, strf = data[slice(*strl[b'strh'])], data[slice(*strl[b'strf'])]
    if strh[:8] != b'vidsMJPG':
        raise ValueError(f'read_avi: the stream is {strh[:8]!r}, not vids / MJPG')
    scale, rate = struct.unpack('<II', strh[20:28])
    w, h = struct.unpack('<ii', strf[4:12])
    movi = top[b'movi'][0] - 4                                                     # the 'movi' word: what idx1 counts from
    streams = []
    for entry in range(top[b'idx1'][0], top[b'idx1'][1], 16):
        fourcc, _, offset, size = struct.unpack('<4sIII', data[entry:entry + 16])
        at = movi + offset
        if fourcc != b'00dc' or data[at:at + 4] != b'00dc' or int.from_bytes(data[at + 4:at + 8], 'little') != size:
            raise ValueError(f'read_avi: the index entry at {entry} does not point at a 00dc chunk of {size} bytes')
        streams.append(data[at + 8:at + 8 + size])
    return streams, (rate // scale if rate % scale == 0 else rate / scale), (w, h)


def decode_avi(path, device=None):
    """``(frames uint8 [F, H, W, 3] on device, fps)`` of a Motion-JPEG AVI: ``decode_jpeg`` of ``read_avi``'s streams — the clip ``save_avi`` wrote, as its
    viewers see it, without a host decoder in the loop."""
    streams, fps, (w, h) = read_avi(path)
    frames = decode_jpeg(streams, device)
    if tuple(frames.shape[1:3]) != (h, w):
        raise ValueError(f'decode_avi: the stream header says {h} x {w}, the frames are {frames.shape[1]} x {frames.shape[2]}')
    return frames, fps


def check_avi(path, frames, quality=90, subsampling='4:2:0'):
    """The dict of ``quality.compare(decode_avi(path)[0], frames)`` plus ``'exact'``: whether the file shows ``jpeg_reconstruct(frames, quality, subsampling)``
    byte for byte — that the clip on disk is the clip the setting promised.  On the frames' device."""
    frames = torch.as_tensor(frames)
    shown = decode_avi(path, frames.device)[0]
    if shown.shape != frames.shape:
        raise ValueError(f'check_avi: the file holds {tuple(shown.shape)}, the frames are {tuple(frames.shape)}')
    metrics = Q.compare(shown, frames)
    metrics['exact'] = bool(torch.equal(shown, jpeg_reconstruct(frames, quality, subsampling)))
    return metrics
