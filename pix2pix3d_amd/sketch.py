"""Sketch sessions: what ``edit.py`` and ``regions.py`` are to the label-map generators, for the edge-map ones (``edge2car``, ``edge2cat``) — an ink canvas to
draw on and erase from, the dataset's preparation of it, edges from any picture or rendered frame, and the cross-view edit.

The reference prepares an edge map on the host with ``cv2`` (``ImageEdgeFolderDataset._load_raw_mask``, training/dataset.py:495-505: ``cv2.blur(255 - file,
(3, 3))`` and a nearest resize) and has no tool that draws one.  Here an INK canvas is uint8 [H, W], 255 = full ink, 0 = paper, and everything is an integer
rule (csrc/sketch/p3d_sketch.h states them; libp3d_sketch.so, a library of its own like the region tools'), each with a torch formulation that CPU tensors
take — the definition — and device kernels whose bytes equal it:

    condition_table(convention)                 float32 [256]: ink value -> conditioning value, in the scripts' own float expressions
    blur3(ink)                                  uint8 [H, W]: the 3 x 3 box blur on reflected taps, (sum + 4) / 9
    condition(ink, resolution, blur, table)     float32 [1, 1, R, R]: blur, nearest resize and table in ONE ``p3d_sketch_condition`` launch
    edge_classes(image, low, high, smooth)      uint8 [H, W] 0 / 1 / 2: luma, [1 4 6 4 1] smoothing, Sobel, non-maximum suppression, two thresholds; one launch
    link(classes)                               uint8 [H, W] 0 / 255: hysteresis — weak pixels survive in an 8-connected component that holds a strong one
    edges(image, low, high, smooth)             ``link(edge_classes(...))``: an ink canvas from any picture or rendered frame
    thin(ink, threshold, passes)                uint8 [H, W] 0 / 255: ``2 * passes`` parallel Zhang-Suen sub-iterations, ping-pong, a fixed count, no readback
    trace(ink, threshold=64, passes)            ``thin`` at the threshold that takes a soft, blurred edge frame back to crisp one-pixel ink
    from_drawing(file_grey)                     ``255 - file``: a dark-on-white drawing as ink

A tap that leaves the image reads the REFLECTED index (``_reflect``: i < 0 -> -i, then i >= n -> 2 n - 2 - i, then clamped to [0, n - 1]; reflect-101, defined
for n = 1 and 2).  Images are uint8 with contiguous pixels and any row pitch, 1 .. 4096 pixels a side; zero-size images return empty results and launch nothing.
``blur3`` alone has no kernel of its own (``condition`` fuses it): it is the torch formulation on the tensor's device.

``SketchSession`` is the edge counterpart of ``edit.EditSession`` on the same stages below the canvas (``edit._StageSession``):

    s = sketch.SketchSession(G, cfg='edge2car')
    s.load(ink, pose)                                     # or s.load_image(photo, pose, low=40, high=120)
    s.pen([(20, 30, 90, 34, 1)]); s.erase([(50, 0, 50, 127, 7)]); s.undo()
    frame = s.frame()                                     # {'image' [H,W,3], 'label' [H,W]} uint8 numpy
    s.set_camera(yaw=40); s.render()                      # neither the Encoder nor the backbone runs
    s.take_view_as_canvas()                               # the rendered edge frame, traced, becomes the canvas
"""
import os

import torch

from . import _lib, edit, views
from .edit import _check_mask
from .resample import resize

_side = _lib.SideLibrary('sketch')                   # libp3d_sketch.so: loaded on the first call, device-guarded; launch_count() is its own counter
SKETCH_LIB_PATH, HEADER = _side.path, _side.header
sketch_lib, launch_count, _check = _side.lib, _side.launch_count, _side.check
MAX_MAGNITUDE, TILE_W, TILE_H = (HEADER.constants[k] for k in ('P3D_SKETCH_MAX_MAGNITUDE', 'P3D_SKETCH_TILE_W', 'P3D_SKETCH_TILE_H'))
THIN_TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc', 'sketch', 'thin_table.h')


def _image_size(image, what):
    """(h, w) of a uint8 [H, W] image with contiguous pixels; (h, w) with a zero for an empty one; ValueError otherwise."""
    if torch.is_tensor(image) and image.dtype == torch.uint8 and image.ndim == 2 and image.numel() == 0:
        return tuple(image.shape)
    return _check_mask(image, what)


def _byte_span(t):
    """[first, past the last) byte address a strided tensor touches."""
    first = t.data_ptr()
    return first, first + (sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1) * t.element_size()


def _out_image(out, h, w, like, inputs, what):
    """A new uint8 [h, w] result, or the caller's ``out`` checked: right size and device, and its byte span apart from every input's (the kernels read
    neighbours while other threads write: a window of the input's own store is refused unless it lies wholly before or after the input's rows)."""
    if out is None:
        return torch.empty([h, w], dtype=torch.uint8, device=like.device)
    if _check_mask(out, 'out') != (h, w) or out.device != like.device:
        raise ValueError(f'{what}: out must be uint8 {h} x {w} on {like.device}')
    lo, hi = _byte_span(out)
    for t in inputs:
        t_lo, t_hi = _byte_span(t)
        if lo < t_hi and t_lo < hi:
            raise ValueError(f'{what} writes out of place: the bytes out spans must not meet an input\'s')
    return out


# ---- reflected taps -------------------------------------------------------------------------------------------------------------------
def _reflect(i, n):
    i = torch.where(i < 0, -i, i)
    i = torch.where(i >= n, 2 * n - 2 - i, i)
    return i.clamp(0, n - 1)


def _tap(img, dy, dx):
    """img[reflect(y + dy)][reflect(x + dx)] for every pixel (x, y) of an int64 [H, W] image."""
    h, w = img.shape
    ys = _reflect(torch.arange(h, device=img.device) + dy, h)
    xs = _reflect(torch.arange(w, device=img.device) + dx, w)
    return img[ys][:, xs]


def _neighbour(img, dy, dx):
    """img[y + dy][x + dx], 0 outside the image."""
    h, w = img.shape
    return torch.nn.functional.pad(img, (1, 1, 1, 1))[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


# ---- ink -> conditioning image -----------------------------------------------------------------------------------------------------------
CONVENTIONS = ('dataset', 'input')


def condition_table(convention='dataset'):
    """float32 [256] on the CPU: the conditioning value of every ink value v, made by the scripts' own torch expressions so that the float bits are theirs.
    'dataset': ``-(v.float() / 127.5 - 1)``, what generate_video.py:198 applies to the dataset's mask (the blurred ink).  'input': ``(255 - v).float() / 127.5 - 1``,
    the scripts' ``--input`` route on a drawing file whose ink is ``255 - file``."""
    v = torch.arange(256, dtype=torch.uint8)
    if convention == 'dataset':
        return -(v.float() / 127.5 - 1)
    if convention == 'input':
        return (255 - v).float() / 127.5 - 1
    raise ValueError(f'condition_table: convention must be one of {CONVENTIONS}, got {convention!r}')


def _as_table(table, device):
    table = condition_table(table) if isinstance(table, str) else table
    if not torch.is_tensor(table) or table.dtype != torch.float32 or tuple(table.shape) != (256,):
        raise ValueError('condition: table must be float32 [256] or the name of a convention')
    return table.to(device).contiguous()


def from_drawing(file_grey):
    """A dark-on-white drawing (uint8, 0 = line) as ink: ``255 - file``."""
    file_grey = torch.as_tensor(file_grey)
    if file_grey.dtype != torch.uint8:
        raise ValueError(f'from_drawing: a uint8 image is needed, got {file_grey.dtype}')
    return 255 - file_grey


def blur3(ink):
    """uint8 [H, W]: m = (sum of the nine reflected taps + 4) / 9 in integers — ``cv2.blur(ink, (3, 3))`` (DESIGN.md section 2.1r derives the equality).  Torch
    integer ops on the tensor's device (``condition`` fuses the blur into its one launch and evaluates it only where the resize looks)."""
    h, w = _image_size(ink, 'ink')
    if h * w == 0:
        return torch.empty([h, w], dtype=torch.uint8, device=ink.device)
    v = ink.long()
    total = sum(_tap(v, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    return ((total + 4) // 9).to(torch.uint8)


def condition(ink, resolution, blur=True, table='dataset'):
    """float32 [1, 1, R, R]: the Encoder's conditioning image of an ink canvas — the optional 3 x 3 blur at source resolution, the nearest resize
    sy = min(y H / R, H - 1), sx = min(x W / R, W - 1) (integer division) and ``table`` (float32 [256], or a convention of ``condition_table``).  Device
    tensors: ONE ``p3d_sketch_condition`` launch; CPU tensors: the torch formulation.  An empty canvas or R = 0 gives an empty image."""
    h, w = _image_size(ink, 'ink')
    r = int(resolution)
    if not 0 <= r <= edit.MAX_SIZE:
        raise ValueError(f'condition: resolution must be 0 .. {edit.MAX_SIZE}, got {resolution!r}')
    table = _as_table(table, ink.device)
    if h * w == 0 or r == 0:
        return torch.empty([1, 1, 0, 0], dtype=torch.float32, device=ink.device)
    if not ink.is_cuda:
        m = blur3(ink) if blur else ink
        sy = (torch.arange(r) * h // r).clamp(max=h - 1)
        sx = (torch.arange(r) * w // r).clamp(max=w - 1)
        return table[m[sy][:, sx].long()][None, None]
    out = torch.empty([1, 1, r, r], dtype=torch.float32, device=ink.device)
    with _lib.kernel_timer('sketch_condition', out):
        code = sketch_lib().p3d_sketch_condition(_lib.ptr(ink), ink.stride(0), h, w, int(bool(blur)), _lib.ptr(table), _lib.ptr(out), out.stride(2), r,
                                                 _lib.stream_of(out))
    _check(code, 'sketch_condition')
    return out


# ---- edges from a picture ----------------------------------------------------------------------------------------------------------------
def _check_thresholds(low, high):
    for v in (low, high):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f'edge_classes: thresholds are integers, got {v!r}')
    if not 0 <= int(low) <= int(high) <= MAX_MAGNITUDE:
        raise ValueError(f'edge_classes: 0 <= low <= high <= {MAX_MAGNITUDE} is needed, got {low}, {high}')
    return int(low), int(high)


def _frame_size(image):
    """(h, w, channels) of a grey uint8 [H, W] or RGB uint8 [H, W, 3] frame with contiguous pixels."""
    if torch.is_tensor(image) and image.dtype == torch.uint8 and image.ndim == 3 and image.shape[2] == 3:
        h, w = image.shape[:2]
        if h * w and (image.stride(2) != 1 or image.stride(1) != 3 or image.stride(0) < 3 * w):
            raise ValueError(f'image: RGB pixels must be contiguous (strides [>= {3 * w}, 3, 1]), got {tuple(image.stride())}')
        if h * w and not (h <= edit.MAX_SIZE and w <= edit.MAX_SIZE):
            raise ValueError(f'image: 1 .. {edit.MAX_SIZE} pixels a side, got {h} x {w}')
        return h, w, 3
    return _image_size(image, 'image') + (1,)


def _edge_classes_torch(image, low, high, smooth):
    v = image.long()
    if v.ndim == 3:
        v = (77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8
    if smooth:
        k = (1, 4, 6, 4, 1)
        rows = sum(k[j + 2] * _tap(v, 0, j) for j in range(-2, 3))
        v = (sum(k[i + 2] * _tap(rows, i, 0) for i in range(-2, 3)) + 128) >> 8
    t = {(dy, dx): _tap(v, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)}
    gx = (t[-1, 1] + 2 * t[0, 1] + t[1, 1]) - (t[-1, -1] + 2 * t[0, -1] + t[1, -1])
    gy = (t[1, -1] + 2 * t[1, 0] + t[1, 1]) - (t[-1, -1] + 2 * t[-1, 0] + t[-1, 1])
    mag = gx.abs() + gy.abs()
    ax, ay = gx.abs(), gy.abs() << 15
    t22 = ax * 13573
    t67 = t22 + (ax << 16)
    n = {(dy, dx): _neighbour(mag, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)}
    across = (mag > n[0, -1]) & (mag >= n[0, 1])
    along = (mag > n[-1, 0]) & (mag >= n[1, 0])
    falling = (mag > n[-1, -1]) & (mag > n[1, 1])                              # s = 1: gx and gy of one sign
    rising = (mag > n[-1, 1]) & (mag > n[1, -1])                               # s = -1
    kept = torch.where(ay < t22, across, torch.where(ay > t67, along, torch.where((gx ^ gy) < 0, rising, falling)))
    return (kept & (mag > low)).to(torch.uint8) + (kept & (mag > high)).to(torch.uint8)


def edge_classes(image, low, high, smooth=True, out=None):
    """uint8 [H, W]: 0 none, 1 weak, 2 strong — of an RGB uint8 [H, W, 3] or grey uint8 [H, W] frame (p3d_sketch.h states the five steps: luma, the optional
    [1 4 6 4 1] smoothing, Sobel with mag = |gx| + |gy|, non-maximum suppression along the gradient's octant, kept and mag > ``high`` / ``low``).
    0 <= low <= high <= 2040.  Device tensors: ONE ``p3d_sketch_edge_classes`` launch; CPU tensors: the torch formulation."""
    h, w, channels = _frame_size(image)
    low, high = _check_thresholds(low, high)
    if h * w == 0:
        return torch.empty([h, w], dtype=torch.uint8, device=image.device)
    out = _out_image(out, h, w, image, (image,), 'edge_classes')
    if not image.is_cuda:
        out.copy_(_edge_classes_torch(image, low, high, bool(smooth)))
        return out
    with _lib.kernel_timer('sketch_edge_classes', out):
        code = sketch_lib().p3d_sketch_edge_classes(_lib.ptr(image), image.stride(0), channels, _lib.ptr(out), out.stride(0), h, w, low, high, int(bool(smooth)),
                                                    _lib.stream_of(out))
    _check(code, 'sketch_edge_classes')
    return out


def link(classes, out=None):
    """uint8 [H, W] 0 / 255: hysteresis.  ink[p] = 255 iff classes[p] != 0 and the 8-connected component of non-zero classes p lies in holds a class-2 pixel.
    Components are ``regions.components(classes != 0, connectivity=8)`` (the existing union-find, three launches of libp3d_regions.so); then, on device
    tensors, ``p3d_sketch_link``: a memset of the flags and two launches (mark, select).  CPU tensors: the same three steps in torch."""
    from . import regions
    h, w = _image_size(classes, 'classes')
    if h * w == 0:
        return torch.empty([h, w], dtype=torch.uint8, device=classes.device)
    out = _out_image(out, h, w, classes, (classes,), 'link')
    ids = regions.components((classes != 0).view(torch.uint8), connectivity=8)
    if not classes.is_cuda:
        flag = torch.zeros(h * w, dtype=torch.bool)
        flag[ids[classes == 2].long()] = True
        out.copy_(((classes != 0) & flag[ids.long()]).to(torch.uint8) * 255)
        return out
    flag = torch.empty([h * w], dtype=torch.int32, device=classes.device)
    with _lib.kernel_timer('sketch_link', out):
        code = sketch_lib().p3d_sketch_link(_lib.ptr(classes), classes.stride(0), _lib.ptr(ids), _lib.ptr(flag), _lib.ptr(out), out.stride(0), h, w,
                                            _lib.stream_of(out))
    _check(code, 'sketch_link')
    return out


def edges(image, low, high, smooth=True):
    """``link(edge_classes(image, low, high, smooth))``: an ink canvas (0 / 255) from any picture or rendered frame."""
    return link(edge_classes(image, low, high, smooth))


# ---- thinning ----------------------------------------------------------------------------------------------------------------------------
NEIGHBOURS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))      # (dy, dx) of N, NE, E, SE, S, SW, W, NW: bit i of the code


def deletable_table():
    """bool [2, 256]: whether a set pixel with the neighbour code (bit i = neighbour i of ``NEIGHBOURS`` is set) is deleted in sub-iteration 0 / 1 of
    Zhang-Suen: 2 <= B <= 6 set neighbours, A == 1 unset -> set steps around the cycle, and N E S == 0 and E S W == 0 (step 0) or N E W == 0 and N S W == 0
    (step 1)."""
    table = torch.zeros([2, 256], dtype=torch.bool)
    for code in range(256):
        p = [(code >> i) & 1 for i in range(8)]
        b, a = sum(p), sum(1 for i in range(8) if not p[i] and p[(i + 1) % 8])
        n, e, s, w = p[0], p[2], p[4], p[6]
        if 2 <= b <= 6 and a == 1:
            table[0, code] = n * e * s == 0 and e * s * w == 0
            table[1, code] = n * e * w == 0 and n * s * w == 0
    return table


def thin_table_header():
    """The text of csrc/sketch/thin_table.h: ``deletable_table`` as 2 x 8 words of 32 bits (``python -m pix2pix3d_amd.sketch`` rewrites the file)."""
    words = [[sum(int(row[32 * k + i]) << i for i in range(32)) for k in range(8)] for row in deletable_table()]
    lines = ['// Zhang-Suen deletable codes: GENERATED by pix2pix3d_amd/sketch.py (python -m pix2pix3d_amd.sketch), do not edit.',
             '// kThinDeletable[step][code / 32] >> (code % 32) & 1: a set pixel with this neighbour code (bit i: neighbour i of N, NE, E, SE, S, SW, W, NW) goes.',
             '#pragma once', '#include <stdint.h>', 'static const uint32_t kThinDeletable[2][8] = {']
    lines += ['    {' + ', '.join(f'0x{v:08x}u' for v in row) + '},' for row in words]
    return '\n'.join(lines + ['};', ''])


def _check_thin(threshold, step_or_passes, what):
    if isinstance(threshold, bool) or int(threshold) != threshold or not 1 <= int(threshold) <= 255:
        raise ValueError(f'{what}: threshold must be an integer 1 .. 255, got {threshold!r}')
    if isinstance(step_or_passes, bool) or int(step_or_passes) != step_or_passes or int(step_or_passes) < 0:
        raise ValueError(f'{what}: a non-negative integer is needed, got {step_or_passes!r}')
    return int(threshold), int(step_or_passes)


_deletable = None     # deletable_table(), made once for the CPU formulation


def thin_step(ink, threshold, step, out=None):
    """One parallel Zhang-Suen sub-iteration (``step`` 0 or 1), out of place: a pixel is set iff ink >= threshold; result = set and not
    ``deletable_table()[step][code]`` ? 255 : 0, neighbours outside the image unset.  Device tensors: ONE ``p3d_sketch_thin_step`` launch."""
    h, w = _image_size(ink, 'ink')
    threshold, step = _check_thin(threshold, step, 'thin_step')
    if step not in (0, 1):
        raise ValueError(f'thin_step: step is 0 or 1, got {step}')
    if h * w == 0:
        return torch.empty([h, w], dtype=torch.uint8, device=ink.device)
    out = _out_image(out, h, w, ink, (ink,), 'thin_step')
    if not ink.is_cuda:
        global _deletable
        if _deletable is None:
            _deletable = deletable_table()
        on = (ink >= threshold).long()
        code = sum(_neighbour(on, dy, dx) << i for i, (dy, dx) in enumerate(NEIGHBOURS))
        out.copy_(((on != 0) & ~_deletable[step][code]).to(torch.uint8) * 255)
        return out
    with _lib.kernel_timer('sketch_thin_step', out):
        code = sketch_lib().p3d_sketch_thin_step(_lib.ptr(ink), ink.stride(0), _lib.ptr(out), out.stride(0), h, w, threshold, step, _lib.stream_of(out))
    _check(code, 'sketch_thin_step')
    return out


def thin(ink, threshold=128, passes=2):
    """uint8 [H, W] 0 / 255: ``passes`` Zhang-Suen iterations = ``2 * passes`` ``thin_step`` launches between two buffers — a fixed count, so nothing is read
    back to decide when to stop.  Two passes take a band three pixels wide to one pixel.  ``passes`` = 0 is the threshold alone (torch)."""
    h, w = _image_size(ink, 'ink')
    threshold, passes = _check_thin(threshold, passes, 'thin')
    if h * w == 0:
        return torch.empty([h, w], dtype=torch.uint8, device=ink.device)
    if passes == 0:
        return (ink >= threshold).to(torch.uint8) * 255
    src, spare = ink, None
    for k in range(2 * passes):
        dst = thin_step(src, threshold, k & 1, out=spare)
        src, spare = dst, (src if k else None)                                 # (the caller's canvas is never a destination)
    return src


def trace(ink, threshold=64, passes=2):
    """``thin`` at the threshold that traces a SOFT edge frame: a one-pixel line that went through the 3 x 3 blur (and a generator) is a band of about 85 of
    255 three pixels wide; everything >= ``threshold`` is the band, two passes leave its one-pixel centre line."""
    return thin(ink, threshold, passes)


# ---- the session -------------------------------------------------------------------------------------------------------------------------
def pen_table(strokes, value):
    """Rows (x0, y0, x1, y1, thickness) as ``edit.stroke_table`` rows with ``value`` (255: ink, 0: paper) for the label: the capsule rule and its limits."""
    t = torch.as_tensor(strokes.cpu() if torch.is_tensor(strokes) else strokes)
    if t.numel() == 0:
        return torch.zeros([0, 6], dtype=torch.int32)
    if t.is_floating_point() or t.dtype == torch.bool or t.ndim != 2 or t.shape[1] != 5:
        raise ValueError(f'strokes must be integers [K, 5] = (x0, y0, x1, y1, thickness), got {t.dtype} {tuple(t.shape)}')
    return edit.stroke_table(torch.cat([t.to(torch.int64), torch.full([t.shape[0], 1], int(value), dtype=torch.int64)], dim=1))


class SketchSession(edit._StageSession):
    """One sketch session on the device ``G`` lives on — the edge counterpart of ``edit.EditSession``; every method runs under ``torch.no_grad()``.

    Stages, each recomputed only when its input changed: canvas (base + stroke log, ONE ``p3d_paint_strokes`` launch per run of new entries) -> conditioning
    image (ONE ``p3d_sketch_condition`` launch) -> ws (``G.mapping``) -> planes -> frame.  ``pen`` / ``erase`` / ``undo`` / ``clear`` / ``load`` /
    ``load_image`` / ``take_view_as_canvas`` dirty the canvas; ``set_seed`` / ``clear_texture`` the ws; a camera change only the frame — neither the
    Encoder nor the backbone runs.

    convention, blur   how the canvas becomes the conditioning image: ``condition_table`` and the dataset's 3 x 3 blur.
    cfg, truncation_psi, jitter, hold_texture, neural_rendering_resolution   as ``edit.EditSession``'s."""

    def __init__(self, G, cfg='edge2car', convention='dataset', blur=True, seed=0, truncation_psi=1, jitter='frozen', hold_texture=True,
                 neural_rendering_resolution=None):
        table = condition_table(convention)
        super().__init__(G, cfg, seed, truncation_psi, jitter, hold_texture, neural_rendering_resolution)
        self.convention, self.blur = convention, bool(blur)
        self._table = table.to(self.device)
        self._log = []                                                         # int32 [k, 6] stroke tables, one per undo step (label 255: pen, 0: erase)
        self._kept = None                                                      # (n, the canvas after the first n entries)
        self._canvas = self._condition = None

    _LOAD = 'load(ink, pose)'

    def _check_generator(self, G):
        if not hasattr(G, 'backbone_planes') or not hasattr(G, 'mapping_label') or getattr(G, 'data_type', None) != 'edge' or getattr(G, 'semantic_channels', 0) != 1:
            raise TypeError(f'SketchSession: {type(G).__name__} is not an edge-map generator (data_type "edge", one label channel) on the one-backbone tri-plane core')

    # -- inputs ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def load(self, ink, pose):
        """``ink`` uint8 [H, W] (numpy or tensor; any size up to 4096 a side: ``condition`` resizes), 255 = full ink; ``pose`` [25]: the item's camera label."""
        ink = torch.as_tensor(ink)
        if ink.dtype != torch.uint8 or ink.ndim != 2 or not (1 <= ink.shape[0] <= edit.MAX_SIZE and 1 <= ink.shape[1] <= edit.MAX_SIZE):
            raise ValueError(f'load: ink must be uint8 [H, W], 1 .. {edit.MAX_SIZE} pixels a side, got {ink.dtype} {tuple(ink.shape)}')
        self._load_pose(pose)
        self._base = ink.to(self.device).contiguous()
        self._log, self._kept = [], None
        self._dirty_canvas()
        self._frame = None

    @torch.no_grad()
    def load_image(self, rgb, pose, low, high, smooth=True):
        """A picture (uint8 [H, W, 3] or grey [H, W]) as the canvas, through ``edges`` on the session's device."""
        rgb = torch.as_tensor(rgb)
        _frame_size(rgb)
        self.load(edges(rgb.to(self.device).contiguous(), low, high, smooth), pose)

    # -- drawing ----------------------------------------------------------------------------------------------------------------
    def pen(self, strokes):
        """Append strokes (x0, y0, x1, y1, thickness) of full ink to the log; one call is one undo step."""
        self._append(pen_table(strokes, 255))

    def erase(self, strokes):
        """Append strokes (x0, y0, x1, y1, thickness) of paper."""
        self._append(pen_table(strokes, 0))

    def _append(self, table):
        self._need_load()
        if sum(len(t) for t in self._log) + len(table) > edit.MAX_STROKES:
            raise ValueError(f'more than {edit.MAX_STROKES} strokes in the log; take_view_as_canvas() or clear() starts a new one')
        if len(table):
            self._log.append(table)
            self._dirty_canvas()

    def undo(self):
        if self._log:
            self._log.pop()
            if self._kept is not None and self._kept[0] > len(self._log):       # the kept canvas holds the entry that went: never a prefix of a later log
                self._kept = None
            self._dirty_canvas()

    def clear(self):
        if self._log:
            self._log, self._kept = [], None
            self._dirty_canvas()

    @property
    def log(self):
        """The stroke tables, oldest first: int32 [k, 6] rows (x0, y0, x1, y1, thickness, 255 or 0)."""
        return tuple(self._log)

    @property
    @torch.no_grad()
    def canvas(self):
        """uint8 [H, W] on the device: the base with the log painted — ONE ``p3d_paint_strokes`` launch over the last kept canvas for the entries that are new
        since (after an ``undo`` behind it: over the base, for the whole log); the base itself while the log is empty.  READ-ONLY: the tensor is the session's
        own (its base or its kept canvas), and writing into it changes the session without dirtying any stage — ``clone()`` it to edit it by hand."""
        self._need_load()
        if self._canvas is None:
            n = len(self._log)
            done, kept = self._kept if self._kept is not None else (0, self._base)      # (undo() and clear() drop a kept canvas that is ahead of the log)
            self._canvas = kept if done == n else edit.paint_strokes(kept, torch.cat(self._log[done:n]))
            self._kept = (n, self._canvas)
        return self._canvas

    # -- stages -----------------------------------------------------------------------------------------------------------------
    def _dirty_canvas(self):
        self._canvas = self._condition = None
        self._dirty_ws()

    @torch.no_grad()
    def condition(self):
        """float32 [1, 1, R, R], R = the mapping network's ``in_resolution``: ONE ``p3d_sketch_condition`` launch on the canvas, kept until it changes."""
        if self._condition is None:
            self._condition = condition(self.canvas, int(self.G.backbone.mapping.in_resolution), blur=self.blur, table=self._table)
        return self._condition

    def _conditioned_ws(self):
        return self.G.mapping(self._z(), edit.forward_label(self.G).to(self.device), {'mask': self.condition(), 'pose': self._pose},
                              truncation_psi=self.truncation_psi)

    def _finish(self, out):
        """{'image' [1,H,W,3], 'label' [1,H,W]} uint8: the output image and the edge frame in grey, as the scripts write edge maps."""
        return views.finish_frames(out, label_mode='grey')

    @torch.no_grad()
    def take_view_as_canvas(self, trace=True, threshold=64, passes=2):
        """The cross-view edit: ``255 -`` the edge frame of the last rendered view — traced back to one-pixel ink unless ``trace`` is off — becomes the base,
        the log empties; nothing leaves the device."""
        ink = 255 - self.render()['label']
        self._base = thin(ink, threshold, passes) if trace else ink            # (``trace`` the function is ``thin`` with these defaults)
        self._log, self._kept = [], None
        self._dirty_canvas()

    _agreement = None                                                          # agreement()'s product: (frame, canvas, arguments, counters, their host copy)

    @torch.no_grad()
    def agreement(self, threshold=128, tolerance=2, trace_passes=2, bins=65):
        """How faithfully the current frame follows the current canvas — the edge counterpart of ``EditSession.agreement``:
        ``evaluate.Agreement.result(tolerance)`` after ``add_ink(self.canvas, trace(255 - frame['label'], passes=trace_passes), threshold)``, the map
        ``take_view_as_canvas`` would take; its 'ink' entry holds the measures.  The canvas must have the frame's size (ValueError otherwise).  Kept with the
        frame: a camera move recomputes it without the Encoder or the backbone, a repeated call launches nothing."""
        from . import evaluate
        self.render()
        frame, canvas, key, kept = self._frame, self.canvas, (int(threshold), int(trace_passes), int(bins)), self._agreement
        if kept is None or kept[0] is not frame or kept[1] is not canvas or kept[2] != key:
            total = evaluate.Agreement(1, self.device, bins)
            evaluate._add_ink_frame(total, canvas, frame['label'], threshold, trace_passes)
            self._agreement = kept = (frame, canvas, key, total, total.host_counters())
        return kept[3].metrics_of(kept[4], tolerance)

    def save(self, directory):
        """Three PNGs: canvas.png (the ink), condition.png (the conditioning image, [-1, 1] as grey) and output.png (the rendered image)."""
        from PIL import Image
        os.makedirs(directory, exist_ok=True)
        Image.fromarray(self.canvas.cpu().numpy()).save(os.path.join(directory, 'canvas.png'))
        grey = ((self.condition()[0, 0].cpu() + 1) * 127.5).round().clamp(0, 255).to(torch.uint8)
        Image.fromarray(grey.numpy()).save(os.path.join(directory, 'condition.png'))
        Image.fromarray(self.render()['image'].cpu().numpy()).save(os.path.join(directory, 'output.png'))


def load_canvas(path, device=None, size=None, filter='box'):
    """uint8 [H, W] on ``device``: the ink that ``SketchSession.save`` wrote as canvas.png (or any 8-bit grey PNG), read and decoded where it will be used
    — ``video.load_png``.  ``size`` ((width, height) or an int): resized to it where it is with ``resample.resize(..., filter)`` (the box filter
    keeps the ink a canvas loses to a nearest lookup).  ValueError for a file that is not 8-bit grey."""
    from . import video
    canvas, info = video.load_png(path, device)
    if info.mode != 'L':
        raise ValueError(f'load_canvas: {path} is mode {info.mode!r}: a canvas is 8-bit grey (L)')
    if size is not None:
        canvas = resize(canvas[None], size, filter)[0]
    return canvas


if __name__ == '__main__':
    with open(THIN_TABLE_PATH, 'w') as f:
        f.write(thin_table_header())
    print(f'wrote {THIN_TABLE_PATH}')
