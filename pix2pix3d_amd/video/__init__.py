"""Video frames encoded on the frames' own device, and the files written from them.  One module per format, each importing only those above it:

    ..clips        what every caller of libp3d_video.so shares: the library, its header, the frame contract (``quality.py`` stands on it too)
    gif            histogram, median cut, box means, dithered indices; ``palettize``, ``save_gif``, ``save_gif_indexed``
    jpeg           baseline JPEG: ``encode_jpeg``, ``save_jpeg``; a decoder's view, ``jpeg_reconstruct``; ``jpeg_quality_for`` (sections 2.1u, 2.1x)
    jpeg_read      the way back from a file: ``jpeg_parse``, ``jpeg_unscan``, ``decode_jpeg``, ``load_jpeg`` (section 2.1y)
    avi            Motion-JPEG AVI: ``save_avi``, ``read_avi``, ``decode_avi``, ``check_avi``
    png            lossless PNG and APNG: ``encode_png``, ``save_png``, ``save_png_sequence``, ``save_apng``, ``png_chunks`` (section 2.1v)
    png_read       the way back from a lossless file: ``png_parse``, ``png_inflate``, ``png_unfilter``, ``decode_png``, ``load_png``, ``decode_apng``,
                   ``check_png``, ``png_rgb`` (section 2.1z)
    clip           ``save_clip``: the one choice among these writers that ``views.generate_video`` and ``surface.geometry_video`` offer

Everywhere the same rule: csrc/video/p3d_video.h states every step in integers, the torch / numpy formulation that CPU tensors take is the definition, and
the device kernels' bytes equal it.  Every public name of the modules is a name of this package."""
from ..clips import HEADER, MAX_PIXELS, VIDEO_LIB_PATH, _side, launch_count, video_lib
from .gif import (BINS, COLORS, MAX_AMPLITUDE, bayer8, box_sums, dither_offsets, histogram, median_cut, palette_from_sums, palette_quality, palettize, quantize,
                  save_gif, save_gif_indexed)
from .jpeg import (JPEG_BLOCK_BITS, JPEG_RESTART, JpegHuffman, encode_jpeg, jpeg_coefficients, jpeg_dct, jpeg_dct_table, jpeg_decode, jpeg_dequantize, jpeg_header,
                   jpeg_huffman, jpeg_idct, jpeg_layout, jpeg_quality_for, jpeg_reconstruct, jpeg_scan, jpeg_tables, jpeg_zigzag, save_jpeg)
from .jpeg_read import (JPEG_LOOKUP_BITS, JPEG_STATUS, JPEG_TABLE_WORDS, JpegInfo, decode_jpeg, jpeg_decode_tables, jpeg_parse, jpeg_status_names, jpeg_unscan,
                        load_jpeg)
from .avi import MAX_AVI_BYTES, check_avi, decode_avi, read_avi, save_avi
from .png import (PNG_ADAPTIVE, PNG_FILTERS, PNG_HEADER_WORDS, PNG_MAX_MATCH, PNG_MODES, PNG_SEGMENT_BYTES, PNG_STATS, PNG_SYMBOLS, depth16, encode_png,
                  png_block_header, png_canonical_codes, png_chunks, png_code_lengths, png_counts, png_deflate, png_filter, png_header, png_segment_rows, save_apng,
                  save_png, save_png_sequence)
from .png_read import (PNG_INFLATE_LANES, PNG_STATUS, PngInfo, check_png, decode_apng, decode_png, load_png, png_inflate, png_parse, png_rgb, png_status_names,
                       png_unfilter)
from .clip import check_clip_options, save_clip
