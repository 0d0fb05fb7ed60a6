"""Interactive editing: the compute core of the reference's ``applications/demo/qt_demo_seg2cat.py`` — paint on a label map, see the 3-D result, turn the
camera, take the rendered label map of the new view back as the canvas, paint again — as a library (no UI).

Per event the demo repaints every stroke ever drawn with ``cv2.line`` on the host and copies the mask to the device, builds the int64 one-hot image, runs the
whole ``G.mapping`` and then the whole ``G.synthesis`` — also when only a camera slider moved and the planes cannot have changed — and finishes the frame in numpy
with a Python loop over 512^2 pixels (:343-399, 429-463).  ``EditSession`` keeps each stage's result until its input changes:

    mask (base + stroke log, ONE ``p3d_paint_strokes`` launch)  ->  geometry ws (``p3d_label_features`` + Encoder)  ->  planes (backbone)  ->  frame

    s = edit.EditSession(G, cfg='seg2cat', seed=0)
    s.load(mask, pose)                                    # uint8 [512, 512] label map, [25] camera label of the dataset item
    s.paint([(200, 260, 300, 250, 35, 2)])                # (x0, y0, x1, y1, thickness, label); one call = one undo step
    frame = s.frame()                                     # {'image' [H,W,3], 'label' [H,W,3], 'label_index' [H,W]} uint8 numpy
    s.set_camera(yaw=60, pitch=50)                        # slider units; only the ray-marcher, the heads and the finishing launch run
    s.render()                                            # the same dict as device tensors
    s.take_view_as_mask()                                 # cross-view edit: the rendered label map becomes the canvas
    s.paint([(250, 300, 260, 340, 20, 4)]); s.undo(); s.save('out/')
    s.scale(4, 1.3); s.remove(5); s.move(('component', 260, 300), 0, -4)   # region tools (regions.py): each call is one undo step too

Stroke coverage (identical bytes on the device kernel and in the torch formulation CPU tensors take).  cv2's polygon fill is not specified, so the rule is
integer: with d = b - a, p = pixel - a, L = d.d, s = p.d, thickness t, all int64, a pixel is covered iff
    s <= 0: 4 |p|^2 <= t^2;    s >= L: 4 |p - d|^2 <= t^2;    otherwise: 4 (p x d)^2 <= t^2 L
— the capsule of radius t / 2 about the segment; a zero-length stroke is a disc; t = 1 strokes are 8-connected and hold both endpoints.  The last stroke in
table order that covers a pixel gives it its label.  Limits (ValueError before any launch): 1 <= t <= 255, 0 <= label <= 255, H, W <= 4096, endpoints in
[-4096, 8191], at most 65 535 strokes; they keep 4 (p x d)^2 below 2^60.

The fast label entry exists for ``MaskMappingNetwork_disentangle`` with ``one_hot=True`` and a 'resnet' Encoder.  ``one_hot=False`` masks and the entangled
mapping networks have float conditioning images (no table): a session serves them through the ordinary ``G.mapping``, staleness tracking unchanged.  The edge
networks have a session of their own, ``sketch.SketchSession`` (an ink canvas instead of a label map); the stages below the canvas are ``_StageSession``, shared.
"""
import contextlib
import copy
import math
import os

import numpy as np
import torch

from . import _lib, mesh, views
from .resample import resize

MAX_SIZE, MAX_STROKES, MIN_COORD, MAX_COORD = _lib.P3D_PAINT_MAX_SIZE, _lib.P3D_PAINT_MAX_STROKES, _lib.P3D_PAINT_MIN_COORD, _lib.P3D_PAINT_MAX_COORD
SLIDER_RANGE = dict(yaw=math.pi / 2, pitch=math.pi, roll=math.pi / 4)         # radians per 100 slider units (qt_demo_seg2cat.py:374-379)
DEMO_RADIUS = 2.7                                                              # (:381)
FORWARD_FOCAL = 4.2647                                                         # (:439)
TEXTURE_FROM = 8                                                               # ws[:, 8:] is the demo's ws_texture (:446-449)


# ---- strokes ------------------------------------------------------------------------------------------------------------------
def stroke_table(strokes):
    """``strokes`` (sequence / array / tensor of (x0, y0, x1, y1, thickness, label)) as a checked int32 [K, 6] CPU tensor."""
    t = torch.as_tensor(np.asarray(strokes.cpu() if torch.is_tensor(strokes) else strokes))
    if t.numel() == 0:
        return torch.zeros([0, 6], dtype=torch.int32)
    if t.is_floating_point() or t.dtype == torch.bool or t.ndim != 2 or t.shape[1] != 6:
        raise ValueError(f'strokes must be integers [K, 6] = (x0, y0, x1, y1, thickness, label), got {t.dtype} {tuple(t.shape)}')
    t = t.to(torch.int64)
    if t.shape[0] > MAX_STROKES:
        raise ValueError(f'at most {MAX_STROKES} strokes per mask, got {t.shape[0]}')
    xy, th, lab = t[:, :4], t[:, 4], t[:, 5]
    if int(xy.min()) < MIN_COORD or int(xy.max()) > MAX_COORD:
        raise ValueError(f'stroke endpoints must lie in [{MIN_COORD}, {MAX_COORD}]')
    if int(th.min()) < 1 or int(th.max()) > 255:
        raise ValueError('stroke thickness must be 1 .. 255')
    if int(lab.min()) < 0 or int(lab.max()) > 255:
        raise ValueError('stroke labels must be 0 .. 255')
    return t.to(torch.int32).contiguous()


def _check_mask(mask, what):
    if not torch.is_tensor(mask) or mask.dtype != torch.uint8 or mask.ndim != 2 or mask.stride(1) != 1 or mask.stride(0) < mask.shape[1]:
        raise ValueError(f'{what} must be a uint8 [H, W] tensor with contiguous rows')
    h, w = mask.shape
    if not (1 <= h <= MAX_SIZE and 1 <= w <= MAX_SIZE):
        raise ValueError(f'{what}: 1 .. {MAX_SIZE} pixels a side, got {h} x {w}')
    return h, w


def _paint_cpu(out, table):
    """The torch formulation of the coverage rule, stroke after stroke, each inside its bounding box (identical bytes)."""
    h, w = out.shape
    for x0, y0, x1, y1, t, label in table.tolist():
        r = (t + 1) // 2
        xa, xb, ya, yb = max(min(x0, x1) - r, 0), min(max(x0, x1) + r, w - 1), max(min(y0, y1) - r, 0), min(max(y0, y1) + r, h - 1)
        if xa > xb or ya > yb:
            continue
        px = torch.arange(xa, xb + 1, dtype=torch.int64)[None, :] - x0
        py = torch.arange(ya, yb + 1, dtype=torch.int64)[:, None] - y0
        dx, dy = x1 - x0, y1 - y0
        big_l, s, t2 = dx * dx + dy * dy, px * dx + py * dy, t * t
        cross = px * dy - py * dx
        cov = torch.where(s <= 0, 4 * (px * px + py * py) <= t2,
                          torch.where(s >= big_l, 4 * ((px - dx) ** 2 + (py - dy) ** 2) <= t2, 4 * cross * cross <= t2 * big_l))
        out[ya:yb + 1, xa:xb + 1][cov] = label


def paint_strokes(base, strokes, out=None):
    """``base`` uint8 [H, W] (rows may be a view of a larger canvas) with ``strokes`` painted in table order -> ``out`` (a new tensor, or the caller's uint8
    [H, W] view, written out of place; bytes around it stay untouched).  Device tensors: ONE ``p3d_paint_strokes`` launch (the checked table is copied to the
    device); CPU tensors: the torch formulation."""
    h, w = _check_mask(base, 'base')
    table = stroke_table(strokes)
    if out is None:
        out = torch.empty([h, w], dtype=torch.uint8, device=base.device)
    elif _check_mask(out, 'out') != (h, w) or out.device != base.device:
        raise ValueError(f'out must be uint8 {h} x {w} on {base.device}')
    if out.data_ptr() == base.data_ptr():
        raise ValueError('paint_strokes writes out of place: out must not be base')
    if not base.is_cuda:
        out.copy_(base)
        _paint_cpu(out, table)
        return out
    dev_table = table.to(base.device) if len(table) else None
    with _lib.kernel_timer('paint_strokes', out):
        code = _lib.lib().p3d_paint_strokes(_lib.ptr(base), base.stride(0), _lib.ptr(out), out.stride(0), h, w, _lib.ptr(dev_table), len(table), _lib.stream_of(out))
    _lib.check(code, 'paint_strokes')
    return out


def replay_order(table, replay):
    """'time': as drawn.  'label': all strokes of label 0, then label 1, ... each in the order drawn — the demo's ``for i in range(6): make_mask`` (:432-433)."""
    if replay not in ('time', 'label'):
        raise ValueError(f"replay must be 'time' or 'label', got {replay!r}")
    if replay == 'time' or len(table) == 0:
        return table
    return table[torch.sort(table[:, 5], stable=True).indices]


# ---- label entry ----------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def label_table(fromrgb, n_labels):
    """float32 [n_labels + 1, C] on the CPU: ``fromrgb`` (the Encoder's first 1x1 ``Conv2dLayer``) applied in fp32 to the n_labels one-hot pixels and, row
    n_labels, to an all-zero pixel.  Made by the layer itself, so its gains, bias, activation and clamp are carried, not restated."""
    if fromrgb.in_channels != n_labels or tuple(fromrgb.weight.shape[2:]) != (1, 1) or fromrgb.up != 1 or fromrgb.down != 1:
        raise ValueError(f'label_table: needs the 1x1 layer over {n_labels} label channels, got {fromrgb}')
    layer = copy.deepcopy(fromrgb).to('cpu', torch.float32)
    pixels = torch.cat([torch.eye(n_labels), torch.zeros(n_labels, 1)], dim=1).reshape(1, n_labels, 1, n_labels + 1)
    return layer(pixels)[0, :, 0, :].t().contiguous()


def label_features(mask, table, dtype=torch.float32, memory_format=torch.contiguous_format):
    """``fromrgb(one_hot(mask))`` without the one-hot image: mask uint8 [N, H, W] (any pitches, contiguous pixels), ``table`` = ``label_table`` on the mask's
    device -> [N, C, H, W] ``dtype`` (fp32 / fp16) in ``memory_format``; out[n, :, y, x] = table[min(mask[n, y, x], L)].  Device tensors: one
    ``p3d_label_features`` launch; CPU tensors: an index."""
    if not torch.is_tensor(mask) or mask.dtype != torch.uint8 or mask.ndim != 3 or mask.stride(2) != 1 or mask.numel() == 0:
        raise ValueError('label_features: mask must be a non-empty uint8 [N, H, W] tensor with contiguous pixels')
    if table.dtype != torch.float32 or table.ndim != 2 or table.shape[0] < 2 or table.shape[0] > 256 or table.shape[1] % 4 or table.device != mask.device:
        raise ValueError(f'label_features: table must be float32 [L + 1, C] (1 <= L <= 255, C % 4 == 0) on {mask.device}, got {table.dtype} {tuple(table.shape)} on {table.device}')
    if dtype not in (torch.float32, torch.float16):
        raise ValueError(f'label_features: dtype must be float32 or float16, got {dtype}')
    n, h, w = mask.shape
    n_labels, c = table.shape[0] - 1, table.shape[1]
    if mask.stride(1) < w or (n > 1 and mask.stride(0) < h * mask.stride(1)):
        raise ValueError('label_features: overlapping mask rows / frames')
    if not mask.is_cuda:
        y = table[mask.long().clamp(max=n_labels)].permute(0, 3, 1, 2).to(dtype)
        return y.contiguous(memory_format=memory_format)
    out = torch.empty([n, c, h, w], dtype=dtype, device=mask.device, memory_format=memory_format)
    table = table.contiguous()
    with _lib.kernel_timer('label_features', out):
        code = _lib.lib().p3d_label_features(_lib.ptr(mask), mask.stride(0), mask.stride(1), _lib.ptr(table), n_labels, _lib.ptr(out), _lib.DTYPE_CODE[dtype],
                                             _lib.i64x4(*out.stride()), n, c, h, w, _lib.stream_of(out))
    _lib.check(code, 'label_features')
    return out


# ---- cameras ------------------------------------------------------------------------------------------------------------------
def camera_from_euler(roll, yaw, pitch, radius=DEMO_RADIUS):
    """float32 [4, 4] cam2world of the demo's sliders in radians (:80-86, 381): the rotation ``Rotation.from_euler('zyx', [roll, yaw, pitch + pi])`` —
    Rx(pitch + pi) Ry(yaw) Rz(roll) — with the camera ``radius`` behind the origin along its own viewing axis."""
    a, b, c = float(roll), float(yaw), float(pitch) + math.pi
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    rx = np.array([[1, 0, 0], [0, math.cos(c), -math.sin(c)], [0, math.sin(c), math.cos(c)]])
    m = np.eye(4)
    m[:3, :3] = rx @ ry @ rz
    m[:3, 3] = -m[:3, 2] * float(radius)
    return torch.from_numpy(m).to(torch.float32)


def slider_angles(yaw=0.0, pitch=0.0, roll=0.0):
    """The demo's slider units (range per 100: yaw pi/2, pitch pi, roll pi/4; :374-379) -> (roll, yaw, pitch) in radians, ``camera_from_euler``'s order."""
    return (roll / 100 * SLIDER_RANGE['roll'], yaw / 100 * SLIDER_RANGE['yaw'], pitch / 100 * SLIDER_RANGE['pitch'])


def forward_label(G):
    """float32 [1, 25]: the forward-facing conditioning pose the demo maps z with (:437-441)."""
    rk = G.rendering_kwargs
    pose = mesh.turntable_poses(rk['avg_camera_pivot'], rk['avg_camera_radius'], n_frames=1, yaw0=3.14 / 2, yaw_range=0.0, pitch_range=0.0, pitch0=3.14 / 2)
    f = FORWARD_FOCAL
    return views.camera_labels(pose, torch.tensor([[f, 0, 0.5], [0, f, 0.5], [0, 0, 1]], dtype=torch.float32))


# ---- the stages below the canvas ----------------------------------------------------------------------------------------------------
class _StageSession:
    """What ``EditSession`` and ``sketch.SketchSession`` share — everything below the canvas: the camera and the loaded pose, the seed and the held texture
    rows, ws -> planes -> frame with staleness, the frozen jitter draws and ``geometry()``.  A subclass brings the canvas (``_base`` and what edits it, calling
    ``_dirty_ws()``), ``_check_generator(G)``, ``_conditioned_ws()`` (the ws of the current canvas and seed, before the texture hold) and ``_finish(out)``
    (one ``G.synthesis`` dict -> the frame dict)."""

    def __init__(self, G, cfg, seed, truncation_psi, jitter, hold_texture, neural_rendering_resolution):
        who = type(self).__name__
        if cfg not in views.VIDEO_CFG:
            raise ValueError(f'{who}: cfg must be one of {sorted(views.VIDEO_CFG)}, got {cfg!r}')
        self._check_generator(G)
        self.G, self.cfg, self.truncation_psi, self.hold_texture = G, cfg, truncation_psi, hold_texture
        self.device = next(G.parameters()).device
        self.nrr = int(views.VIDEO_CFG[cfg]['neural_rendering_resolution'] if neural_rendering_resolution is None else neural_rendering_resolution)
        rk = G.rendering_kwargs
        m, sc, sf = self.nrr * self.nrr, int(rk['depth_resolution']), int(rk['depth_resolution_importance'])
        if isinstance(jitter, (tuple, list)):
            self._draws = tuple(torch.as_tensor(u, dtype=torch.float32).to(self.device) for u in jitter)
            if tuple(self._draws[0].shape) != (1, m, sc, 1) or tuple(self._draws[1].shape) != (m, sf):
                raise ValueError(f'{who}: frozen draws must be [1, {m}, {sc}, 1] and [{m}, {sf}]')
        elif jitter == 'frozen':
            self._draws = (torch.rand([1, m, sc, 1], device=self.device), torch.rand([m, sf], device=self.device))
        elif jitter == 'random':
            self._draws = None
        else:
            raise ValueError(f"{who}: jitter must be 'frozen', 'random' or a pair of draws, got {jitter!r}")
        self.palette = None
        self._base = self._pose = self._intrinsics = self._cam2world = None
        self._ws = self._held = self._planes = self._frame = self._floats = None
        self.seed = int(seed)

    def _load_pose(self, pose):
        """``pose`` [25], the item's camera label: its intrinsics serve every later camera (:335) and it is the first camera."""
        pose = torch.as_tensor(pose, dtype=torch.float32).reshape(-1)
        if pose.numel() != 25:
            raise ValueError(f'load: pose must hold 25 floats, got {pose.numel()}')
        self._pose = pose.to(self.device).reshape(1, 25)
        self._intrinsics = self._pose[:, 16:25].reshape(3, 3)
        self._cam2world = self._pose[:, :16].reshape(4, 4)

    def set_seed(self, seed):
        if int(seed) != self.seed:
            self.seed = int(seed)
            self._dirty_ws()

    def clear_texture(self):
        """Release the held ``ws[:, 8:]``: the next ``encode()`` takes the appearance rows of the current seed and holds those."""
        self._held = None
        self._dirty_ws()

    # -- cameras ----------------------------------------------------------------------------------------------------------------
    def set_camera(self, yaw=0.0, pitch=0.0, roll=0.0, radius=DEMO_RADIUS):
        """The demo's three sliders (units of 1/100 of pi/2, pi and pi/4)."""
        self.set_pose(camera_from_euler(*slider_angles(yaw, pitch, roll), radius=radius))

    def set_pose(self, cam2world):
        cam2world = torch.as_tensor(cam2world, dtype=torch.float32).reshape(4, 4).to(self.device)
        self._need_load()
        if not torch.equal(cam2world, self._cam2world):
            self._cam2world = cam2world
            self._frame = None

    @property
    def camera(self):
        """float32 [1, 25]: the current pose with the loaded item's intrinsics."""
        self._need_load()
        return views.camera_labels(self._cam2world, self._intrinsics)

    # -- stages -----------------------------------------------------------------------------------------------------------------
    _LOAD = 'load(...)'                                                        # the subclass's own signature, for the message below

    def _need_load(self):
        if self._base is None:
            raise RuntimeError(f'{type(self).__name__}: {self._LOAD} first')

    def _dirty_ws(self):
        self._ws = self._planes = self._frame = None

    def _z(self):
        return torch.from_numpy(np.random.RandomState(self.seed).randn(1, self.G.z_dim).astype('float32')).to(self.device)      # (:430)

    @torch.no_grad()
    def encode(self):
        """``ws`` [1, num_ws, w_dim]: geometry rows from the canvas, appearance rows from z(seed) under the forward-facing conditioning pose, truncated as
        ``G.mapping`` does; with ``hold_texture`` rows 8.. are those of the first encode."""
        if self._ws is not None:
            return self._ws
        ws = self._conditioned_ws()
        if self.hold_texture:
            if self._held is None:
                self._held = ws[:, TEXTURE_FROM:].clone()
            else:
                ws = torch.cat([ws[:, :TEXTURE_FROM], self._held], dim=1)
        self._ws = ws
        return ws

    @torch.no_grad()
    def render(self, return_float=False):
        """The frame dict of ``_finish`` as uint8 tensors on the device; with ``return_float`` also 'float', the ``G.synthesis`` dict the frame was finished
        from.  Planes and frame are kept: after a camera change this is ``G.synthesis(ws, c, use_cached_backbone=True)`` on the kept planes and the finishing
        launch — neither the Encoder nor the backbone runs."""
        ws, G = self.encode(), self.G
        if self._planes is None:
            self._planes = G.backbone_planes(ws, noise_mode='const')
        if self._frame is None:
            found, G._last_planes = G._last_planes, self._planes
            try:
                draws = views._frozen_draws(self._draws[0], self._draws[1]) if self._draws is not None else contextlib.nullcontext()
                with draws:
                    out = G.synthesis(ws, self.camera, neural_rendering_resolution=self.nrr, use_cached_backbone=True, noise_mode='const')
            finally:
                G._last_planes = found
            self._frame = {k: v[0] for k, v in self._finish(out).items()}
            self._floats = out
        return dict(self._frame, float=self._floats) if return_float else dict(self._frame)

    def frame(self):
        """``render()`` on the host, as numpy arrays."""
        return {k: v.cpu().numpy() for k, v in self.render().items()}

    _surface = None                                                            # geometry()'s product: (planes, cam2world, arguments, frame)

    @torch.no_grad()
    def geometry(self, resolution=None, color='grey', **cast_kwargs):
        """uint8 [R, R, 3] on the device: the SHAPE the current edit produced, seen from the current camera — ``surface.render`` on the kept planes
        (R = ``resolution``, default ``G.img_resolution``; ``color`` and ``cast_kwargs`` as there).  A fifth kept product: it is recomputed when the planes
        or the camera were replaced (whatever dirties them dirties it) or the arguments differ; a camera move runs one cast launch and the shade launch,
        neither the Encoder nor the backbone ('rgb' / 'label' colours query ``G.sample_mixed``, which does run the backbone)."""
        from . import surface
        ws, G = self.encode(), self.G
        if self._planes is None:
            self._planes = G.backbone_planes(ws, noise_mode='const')
        res = int(G.img_resolution if resolution is None else resolution)
        key = (res, color, sorted(cast_kwargs.items()))
        kept = self._surface
        if kept is None or kept[0] is not self._planes or kept[1] is not self._cam2world or kept[2] != key:
            frame = surface.render(G, ws, self.camera, res, color=color, palette=self.palette, planes=self._planes, **cast_kwargs)[0]
            self._surface = kept = (self._planes, self._cam2world, key, frame)
        return kept[3]

    @torch.no_grad()
    def consistency(self, yaw=0.0, pitch=0.0, roll=0.0, tolerance=None, radius=0):
        """How well the current frame agrees in 3D with a second view of the same planes: the current camera turned about the generator's camera pivot by
        ``yaw`` / ``pitch`` / ``roll`` RADIANS (``reproject.turned_camera``) is rendered by one extra ``G.synthesis(..., use_cached_backbone=True)`` on the kept
        planes — neither the Encoder nor the backbone runs —, both views become frames at the neural rendering resolution (``reproject.raw_frames``) and the
        current one is warped into the second: ``reproject.consistency_counts(..., pairs=[(0, 1)])``.  Returns ``reproject.Consistency.result()`` with
        'tolerance' (default ``reproject.default_tolerance(G)``) and 'views', the dict of what was compared ('labels', 'images', 'depth', 'cameras')."""
        from . import reproject
        G = self.G
        first = self.render(return_float=True)['float']
        cams = torch.cat([self.camera, reproject.turned_camera(self.camera, G.rendering_kwargs['avg_camera_pivot'], yaw, pitch, roll)])
        found, G._last_planes = G._last_planes, self._planes
        try:
            with views._frozen_draws(self._draws[0], self._draws[1]) if self._draws is not None else contextlib.nullcontext():
                second = G.synthesis(self.encode(), cams[1:], neural_rendering_resolution=self.nrr, use_cached_backbone=True, noise_mode='const')
        finally:
            G._last_planes = found
        both = reproject.raw_frames({k: torch.cat([first[k], second[k]]) for k in ('image_raw', 'image_depth', 'semantic_raw') if k in first})
        tolerance = reproject.default_tolerance(G) if tolerance is None else tolerance
        total = reproject.consistency_counts(both['labels'], both['images'], both['depth'], cams, [(0, 1)], both['n_labels'], tolerance, radius)
        out = total.result()
        out.update(tolerance=int(tolerance), views=dict(both, cameras=cams))
        return out


# ---- the session ----------------------------------------------------------------------------------------------------------------
class EditSession(_StageSession):
    """One editing session on the device ``G`` lives on; every method runs under ``torch.no_grad()``.

    Four stages, each recomputed only when its input changed: mask -> geometry ws -> planes -> frame (and, beside the frame, ``geometry()``'s surface frame).  ``paint`` / ``undo`` / ``clear`` / ``load`` /
    ``take_view_as_mask`` and the region tools (``fill`` / ``grow`` / ``shrink`` / ``remove`` / ``move`` / ``scale`` / ``rotate`` / ``transform``) dirty the mask;
    ``set_seed`` / ``clear_texture`` the ws; a camera change only the frame: ``render()`` after it is
    ``G.synthesis(ws, c, use_cached_backbone=True)`` on the kept planes and ``views.finish_frames`` — neither the Encoder nor the backbone runs.

    cfg            a key of ``views.VIDEO_CFG``: the ray resolution (``neural_rendering_resolution`` overrides it).
    truncation_psi as ``G.mapping``'s.
    jitter         'frozen' (one set of stratified draws for the whole session: a frame changes only with its inputs), 'random', or a pair of draws, as
                   ``views.render_views``.
    hold_texture   keep ``ws[:, 8:]`` of the first ``encode()`` until ``clear_texture()`` — the demo's ``ws_texture`` (:446-449).
    replay         'time': strokes in the order drawn; 'label': the demo's order, label by label (:432-433)."""

    def __init__(self, G, cfg='seg2cat', seed=0, truncation_psi=1, jitter='frozen', hold_texture=True, replay='time', neural_rendering_resolution=None,
                 palette=None):
        super().__init__(G, cfg, seed, truncation_psi, jitter, hold_texture, neural_rendering_resolution)
        replay_order(torch.zeros([0, 6], dtype=torch.int32), replay)
        self.replay = replay
        self.n_labels = int(G.semantic_channels)
        self.palette = mesh.default_palette(self.n_labels) if palette is None else torch.as_tensor(palette)
        if self.device.type == 'cuda':
            self.palette = self.palette.to(self.device)                        # read in place by every finishing launch
        mapping = G.backbone.mapping
        self.fast_entry = hasattr(mapping, 'geometry_ws') and getattr(mapping, 'one_hot', False) and mapping.embed_mask.architecture == 'resnet' \
            and not mapping.embed_mask.progressive
        self._table = None
        if self.fast_entry:
            enc = mapping.embed_mask
            self._table = label_table(getattr(enc, f'b{enc.block_resolutions[0]}').fromrgb, self.n_labels).to(self.device)
        self._forward_c = G.mapping_label(forward_label(G).to(self.device))
        self._log = []                                                         # typed entries, one per undo step: ('paint', int32 [k, 6] table) or a region op
        self._kept = {}                                                        # n -> the mask after the first n entries (at most KEPT_MASKS of them)
        self._mask = self._geometry = None
        self._appearance = {}                                                  # seed -> [1, w_dim]

    _LOAD = 'load(mask, pose)'

    def _check_generator(self, G):
        if not hasattr(G, 'backbone_planes') or not hasattr(G, 'mapping_label') or not hasattr(G, 'semantic_channels') or G.semantic_channels < 2:
            raise TypeError(f'EditSession: {type(G).__name__} is not a label-map generator on the one-backbone tri-plane core')

    # -- inputs ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def load(self, mask, pose):
        """``mask`` uint8 [H, W] (numpy or tensor), H = W = the mapping network's ``in_resolution``, every label < ``semantic_channels`` (checked here, once, on
        the host); ``pose`` [25]: the item's camera label — its intrinsics serve every later camera (:335) and it is the first camera."""
        mask = torch.as_tensor(mask)
        res = int(self.G.backbone.mapping.in_resolution)
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (res, res):
            raise ValueError(f'load: mask must be uint8 [{res}, {res}], got {mask.dtype} {tuple(mask.shape)}')
        if int(mask.max()) >= self.n_labels:
            raise ValueError(f'load: label {int(mask.max())} in a mask of {self.n_labels} labels')
        self._load_pose(pose)
        self._base = mask.to(self.device).contiguous()
        self._log, self._kept = [], {}
        self._dirty_mask()
        self._frame = None

    # -- painting ---------------------------------------------------------------------------------------------------------------
    def paint(self, strokes):
        """Append strokes (x0, y0, x1, y1, thickness, label) to the log; one call is one undo step."""
        table = stroke_table(strokes)
        if len(table) and int(table[:, 5].max()) >= self.n_labels:
            raise ValueError(f'paint: label {int(table[:, 5].max())} in a mask of {self.n_labels} labels')
        if sum(len(e[1]) for e in self._log if e[0] == 'paint') + len(table) > MAX_STROKES:
            raise ValueError(f'paint: more than {MAX_STROKES} strokes in the log; take_view_as_mask() or clear() starts a new one')
        if len(table):
            self._append(('paint', table))

    def undo(self):
        if self._log:
            self._log.pop()
            self._kept = {n: m for n, m in self._kept.items() if n <= len(self._log)}
            self._dirty_mask()

    def clear(self):
        if self._log:
            self._log, self._kept = [], {}
            self._dirty_mask()

    def _append(self, entry):
        self._log.append(entry)
        self._dirty_mask()

    # -- region tools (regions.py): every call validates on the host, appends ONE entry and dirties the mask as paint() does -------------------------
    def _own_label(self, label, what):
        if isinstance(label, bool) or not isinstance(label, (int, np.integer)) or not 0 <= int(label) < self.n_labels:
            raise ValueError(f'{what}: label {label!r} in a mask of {self.n_labels} labels')
        return int(label)

    def _pixel(self, x, y, what):
        self._need_load()
        h, w = self._base.shape
        if not all(isinstance(v, (int, np.integer)) for v in (x, y)) or not (0 <= x < w and 0 <= y < h):
            raise ValueError(f'{what}: pixel ({x!r}, {y!r}) is outside the {h} x {w} mask')
        return int(x), int(y)

    def _region_spec(self, region, what):
        """A label, or ('component', x, y[, connectivity]): resolved against the mask when the entry is applied."""
        if isinstance(region, (tuple, list)):
            if len(region) not in (3, 4) or region[0] != 'component' or (len(region) == 4 and region[3] not in (4, 8)):
                raise ValueError(f"{what}: a region is a label or ('component', x, y[, 4 or 8]), got {region!r}")
            return ('component',) + self._pixel(region[1], region[2], what) + (int(region[3]) if len(region) == 4 else 4,)
        return self._own_label(region, what)

    def _resolve(self, mask, spec):
        from . import regions
        return regions.select(mask, *spec[1:]) if isinstance(spec, tuple) else mask == spec

    def _centre(self, spec, centre):
        """``centre`` (x, y), or the centre of the region's bounding box in the current mask — read once, here (one host synchronisation)."""
        if centre is not None:
            cx, cy = (float(v) for v in centre)
            return cx, cy
        from . import regions
        box = regions.bbox(self._resolve(self.mask, spec))
        return (0.0, 0.0) if box is None else ((box[0] + box[2]) / 2, (box[1] + box[3]) / 2)

    def fill(self, x, y, label, connectivity=4):
        """Bucket fill: ``label`` over the component of pixel (x, y)."""
        if connectivity not in (4, 8):
            raise ValueError(f'fill: connectivity must be 4 or 8, got {connectivity!r}')
        self._append(('fill',) + self._pixel(x, y, 'fill') + (self._own_label(label, 'fill'), connectivity))

    def grow(self, label, radius, over=None):
        """Dilate ``label`` by the disc of ``radius`` pixels; ``over``: the labels it may grow over (default: all)."""
        label, over = self._own_label(label, 'grow'), None if over is None else tuple(sorted({self._own_label(l, 'grow') for l in over}))
        self._append(('grow', label, self._radius(radius, 'grow'), over))

    def shrink(self, label, radius):
        """Erode ``label`` by the disc of ``radius`` pixels; the vacated pixels take the nearest other label."""
        self._append(('shrink', self._own_label(label, 'shrink'), self._radius(radius, 'shrink')))

    def remove(self, label):
        """The label disappears under its nearest surroundings (``shrink`` without a bound)."""
        self._append(('shrink', self._own_label(label, 'remove'), -1))

    def _radius(self, radius, what):
        self._need_load()
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= MAX_SIZE:
            raise ValueError(f'{what}: radius must be an integer 0 .. {MAX_SIZE}, got {radius!r}')
        return int(radius)

    def move(self, region, dx, dy):
        """Shift the region by (dx, dy) pixels (y grows downwards); what it vacates is filled from the nearest surroundings."""
        self.transform(region, [[1, 0, dx], [0, 1, dy]])

    def scale(self, region, factor, centre=None):
        """Scale the region by ``factor`` (a number, or (fx, fy)) about ``centre`` (x, y; default: the centre of its bounding box in the current mask)."""
        spec = self._region_spec(region, 'scale')
        fx, fy = (float(v) for v in factor) if isinstance(factor, (tuple, list)) else (float(factor), float(factor))
        cx, cy = self._centre(spec, centre)
        self.transform(spec, [[fx, 0, cx - fx * cx], [0, fy, cy - fy * cy]])

    def rotate(self, region, degrees, centre=None):
        """Rotate the region by ``degrees`` about ``centre`` (as ``scale``'s): (x, y) -> (x cos - y sin, x sin + y cos) in pixel axes, y downwards."""
        spec = self._region_spec(region, 'rotate')
        c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
        cx, cy = self._centre(spec, centre)
        self.transform(spec, [[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy]])

    def transform(self, region, matrix, fill='nearest'):
        """Move the region by the forward 2 x 3 ``matrix``; ``fill`` as ``regions.transform``.  The entry stores the six integers of ``regions.affine_coef``,
        neither the floats nor a centre: a replay never depends on float arithmetic."""
        from . import regions
        self._need_load()
        spec = self._region_spec(region, 'transform')
        if isinstance(fill, str):
            if fill != 'nearest':
                raise ValueError(f"transform: fill must be 'nearest' or a label, got {fill!r}")
        else:
            fill = self._own_label(fill, 'transform')
        self._append(('warp', spec, regions.affine_coef(matrix), fill))

    def _apply(self, mask, entry):
        from . import regions
        kind = entry[0]
        if kind == 'fill':
            return regions.flood_fill(mask, *entry[1:])
        if kind == 'grow':
            return regions.grow(mask, *entry[1:])
        if kind == 'shrink':
            return regions.shrink(mask, *entry[1:])
        return regions.transform(mask, self._resolve(mask, entry[1]), entry[2], fill=entry[3])

    @property
    def log(self):
        """The entries, oldest first: ('paint', table), ('fill', x, y, label, connectivity), ('grow', label, radius, over), ('shrink', label, radius — -1: remove),
        ('warp', region, six integers, fill)."""
        return tuple(self._log)

    @property
    def strokes(self):
        """Every stroke of the log as one int32 [K, 6] CPU table, in the order a run of paint() calls is painted in."""
        tables = [e[1] for e in self._log if e[0] == 'paint']
        table = torch.cat(tables) if tables else torch.zeros([0, 6], dtype=torch.int32)
        return replay_order(table, self.replay)

    KEPT_MASKS = 32

    def _mask_after(self, n):
        """The mask after the first ``n`` entries.  A maximal run of paint entries is ONE ``p3d_paint_strokes`` launch over the mask in front of the run (``replay``
        orders the strokes inside it); any other entry runs on the mask in front of it.  Masks are kept, so appending an entry runs that entry alone (a paint entry: its run,
        one launch) and ``undo()`` back to a mask that was read runs nothing; past ``KEPT_MASKS`` the oldest are dropped and replay from the nearest kept one."""
        todo = []                                                              # (first entry, end) segments still to apply, newest first
        while n > 0 and n not in self._kept:
            first = n - 1
            while self._log[n - 1][0] == 'paint' and first > 0 and self._log[first - 1][0] == 'paint':
                first -= 1
            todo.append((first, n))
            n = first
        mask = self._kept[n] if n else self._base
        for first, end in reversed(todo):
            if self._log[first][0] == 'paint':
                mask = paint_strokes(mask, replay_order(torch.cat([e[1] for e in self._log[first:end]]), self.replay))
            else:
                mask = self._apply(mask, self._log[first])
            self._kept[end] = mask
            while len(self._kept) > self.KEPT_MASKS:
                del self._kept[min(self._kept)]
        return mask

    @property
    @torch.no_grad()
    def mask(self):
        """uint8 [H, W] on the device: the base with the log applied (the launches of the entries that are new since the last kept mask; the base itself
        while the log is empty)."""
        self._need_load()
        if self._mask is None:
            self._mask = self._mask_after(len(self._log))
        return self._mask

    # -- stages (the camera, encode(), render(), frame() and geometry() are the base class's) -------------------------------------------------------
    def _dirty_mask(self):
        self._mask = self._geometry = None
        self._dirty_ws()

    def _conditioned_ws(self):
        """Geometry rows from the mask (the label entry and the Encoder, kept until the mask changes), appearance rows from z(seed) under the forward-facing
        conditioning pose (cached per seed), truncated as ``G.mapping`` does."""
        mask, mapping = self.mask, self.G.backbone.mapping
        if self.fast_entry:
            from .training.networks_stylegan2 import truncate_ws
            if self._geometry is None:
                self._geometry = mapping.geometry_ws(mask[None], self._table)
            if self.seed not in self._appearance:
                self._appearance[self.seed] = mapping.appearance_w(self._z(), self._forward_c)
            w = self._appearance[self.seed]
            ws = torch.cat([self._geometry, w.unsqueeze(1).repeat([1, mapping.num_ws - mapping.geometry_layer, 1])], dim=1)
            ws = truncate_ws(mapping, ws, self.truncation_psi, None)
        else:
            ws = self.G.mapping(self._z(), forward_label(self.G).to(self.device), {'mask': mask[None, None], 'pose': self._pose}, truncation_psi=self.truncation_psi)
        return ws

    def _finish(self, out):
        """{'image' [1,H,W,3], 'label' [1,H,W,3], 'label_index' [1,H,W]} uint8 — the demo's output image, its coloured label map and its ``buffer_mask``."""
        return views.finish_frames(out, palette=self.palette, label_mode='palette')

    @torch.no_grad()
    def take_view_as_mask(self):
        """The cross-view edit (``get_mask``, :343-349): the label map of the last rendered view becomes the base, the log empties; nothing leaves the device."""
        base = self.render()['label_index']
        res = int(self.G.backbone.mapping.in_resolution)
        if tuple(base.shape) != (res, res):
            raise ValueError(f'take_view_as_mask: the rendered label map is {tuple(base.shape)}, the mapping network takes {res} x {res}')
        self._base, self._log, self._kept = base.clone(), [], {}
        self._dirty_mask()

    _agreement = None                                                          # agreement()'s product: (frame, mask, bins, counters, their host copy)

    @torch.no_grad()
    def agreement(self, tolerance=2, bins=65):
        """How faithfully the current frame follows the current mask: ``evaluate.Agreement.result(tolerance)`` of ``self.mask`` against
        ``self.render()['label_index']`` at the current camera (``n_labels`` is the generator's).  Kept with the frame: whatever replaces the frame (an edit,
        a seed, a camera move) recomputes it — after a camera move without the Encoder or the backbone —, a repeated call launches nothing and copies nothing."""
        from . import evaluate
        self.render()
        frame, mask, kept = self._frame, self.mask, self._agreement
        if kept is None or kept[0] is not frame or kept[1] is not mask or kept[2] != int(bins):
            total = evaluate.Agreement(self.n_labels, self.device, bins)
            evaluate._add_label_frame(total, mask, frame['label_index'])
            self._agreement = kept = (frame, mask, int(bins), total, total.host_counters())
        return kept[3].metrics_of(kept[4], tolerance)

    def save(self, directory):
        """The demo's three PNGs (:465-472): mask.png (labels), mask_color.png (palette colours), output.png (the rendered image)."""
        from PIL import Image
        os.makedirs(directory, exist_ok=True)
        mask = self.mask.cpu()
        Image.fromarray(mask.numpy()).save(os.path.join(directory, 'mask.png'))
        Image.fromarray(self.palette.cpu()[mask.long()].numpy()).save(os.path.join(directory, 'mask_color.png'))
        Image.fromarray(self.render()['image'].cpu().numpy()).save(os.path.join(directory, 'output.png'))


def load_mask(path, device=None, size=None):
    """uint8 [H, W] on ``device``: the label map that ``EditSession.save`` wrote as mask.png (or any 8-bit grey PNG), read and decoded where it will be
    used — ``video.load_png``: no PIL, no numpy array, no second upload.  ``size`` ((width, height) or an int): resized to it where it is with
    ``resample.resize(..., 'nearest')`` — a label is never blended — so that a map of any size enters a session.  ValueError for a file that is not 8-bit grey."""
    from . import video
    mask, info = video.load_png(path, device)
    if info.mode != 'L':
        raise ValueError(f'load_mask: {path} is mode {info.mode!r}: a label map is 8-bit grey (L)')
    if size is not None:
        mask = resize(mask[None], size, 'nearest')[0]
    return mask
