"""What a synthesis pass does on the device, as an ordered list of small records (tests/golden/block_routes.json holds the ones the commit before
modconv.block_route made; tests/test_block_route*.py compare with them):

    ['block', {...}]                            a SynthesisBlock.forward begins: the numbers modconv.block_route decides from
    ['call', symbol, 'side' | 'main' | None, [...]]   one C ABI call through _lib.lib(): the stream it was given (the device's prefetch stream, or the calling
                                                stream; None: the entry point takes none), then every scalar argument's value and 'ptr' / 'null' for every
                                                pointer, in the order of include/p3d_hip.h (``param_names(symbol)`` gives the names)
    ['wait_event' | 'wait_stream', 'side' | 'main']   torch.cuda.Stream.wait_event / wait_stream, and which stream waits
    ['wrapper', name, [n, ci, h, w]]            modconv.conv3x3_torgb_wide / torgb_wide_skip / conv3x3_torgb / torgb, and the shape of its activations
    ['split', [n, c, h, w]]                     SplitActs.__init__

A plain helper: it patches for the duration of a ``with`` and puts everything back."""
import ctypes
import hashlib
import json
import os

import torch

from conftest import GOLDEN

WRAPPERS = ('conv3x3_torgb_wide', 'torgb_wide_skip', 'conv3x3_torgb', 'torgb')
OUTPUTS = ('image', 'image_raw', 'semantic', 'semantic_raw', 'image_depth')
GOLDEN_FILE = os.path.join(GOLDEN, 'block_routes.json')

_names = {}


def param_names(symbol):
    """The parameter names of a C ABI entry point, read from the header with _lib.Header's own declarator parser."""
    from pix2pix3d_amd import _lib
    if not _names:
        class Named(_lib.Header):
            def _declare(self, sym, text, ctype='', member=False):
                out = super()._declare(sym, text, ctype, member)
                if not member:
                    _names.setdefault(sym, []).append(out[0])
                return out
        header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), 'include', 'p3d_hip.h')
        with open(header) as f:
            Named(f.read())
    return _names.get(symbol, [])


def arg_names(symbol):
    """... without the stream: the names of what a 'call' record's last slot lists."""
    return [n for n in param_names(symbol) if n != 'stream']


def _scalar(v):
    v = getattr(v, 'value', v)
    return float(v) if isinstance(v, float) else int(v)


def _is_null(v):
    if v is None:
        return True
    if isinstance(v, ctypes.c_void_p):
        return not v.value
    return isinstance(v, int) and v == 0


class Tracer:
    """``with Tracer() as t: ...`` -> ``t.events``.  ``skip_image=(block, fn)``: that block is handed ``fn(img)`` for its skip image."""

    def __init__(self, skip_image=None):
        self.events, self.skip_image = [], skip_image

    def _stream_name(self, handle):
        from pix2pix3d_amd.torch_utils.ops import modconv
        return 'side' if any(p.side.cuda_stream == handle for p in modconv._plans.values()) else 'main'

    def __enter__(self):
        from pix2pix3d_amd import _lib
        from pix2pix3d_amd.torch_utils.ops import modconv
        from pix2pix3d_amd.training import networks_stylegan2 as ns
        events, tracer = self.events, self
        real_lib = _lib.lib()

        class Recording:
            def __getattr__(proxy, symbol):
                fn, names, types = getattr(real_lib, symbol), param_names(symbol), _lib.HEADER.functions[symbol][1]

                def call(*args):
                    stream, values = None, []
                    for name, ctype, v in zip(names, types, args):
                        if name == 'stream':
                            stream = tracer._stream_name(getattr(v, 'value', v) or 0)
                        elif ctype is ctypes.c_void_p:
                            values.append('null' if _is_null(v) else 'ptr')
                        else:
                            values.append(float(_scalar(v)) if ctype in (ctypes.c_float, ctypes.c_double) else _scalar(v))
                    events.append(['call', symbol, stream, values])
                    return fn(*args)
                return call
        self._guarded, _lib._guarded = _lib._guarded, Recording()

        self._waits = (torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream)

        def wait_event(stream, ev, _real=self._waits[0]):
            events.append(['wait_event', tracer._stream_name(stream.cuda_stream)])
            return _real(stream, ev)

        def wait_stream(stream, other, _real=self._waits[1]):
            events.append(['wait_stream', tracer._stream_name(stream.cuda_stream)])
            return _real(stream, other)
        torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream = wait_event, wait_stream

        self._wrappers = {name: getattr(modconv, name) for name in WRAPPERS}
        for name, real in self._wrappers.items():
            def wrapper(x, *args, _name=name, _real=real, **kwargs):
                events.append(['wrapper', _name, list(x.shape)])
                return _real(x, *args, **kwargs)
            setattr(modconv, name, wrapper)

        self._split_init = modconv.SplitActs.__init__

        def split_init(acts, t, _real=self._split_init):
            events.append(['split', list(t.shape)])
            return _real(acts, t)
        modconv.SplitActs.__init__ = split_init

        cls = ns.SynthesisBlock
        self._own_forward = cls.__dict__.get('forward')
        real_forward = cls.forward

        def forward(block, x, img, ws, force_fp32=False, fused_modconv=None, update_emas=False, _split_ok=False, _x_dead=False, **layer_kwargs):
            dtype, fmt, fused = ns._block_mode(block, ws, force_fp32, fused_modconv)
            events.append(['block', dict(
                batch=int(ws.shape[0]), in_channels=block.in_channels, out_channels=block.conv1.out_channels, img_channels=block.img_channels,
                resolution=block.resolution, in_div=block._in_div, dtype=str(dtype).replace('torch.', ''), channels_last=fmt == torch.channels_last,
                architecture=block.architecture, is_last=bool(block.is_last), fused_modconv=fused if isinstance(fused, bool) else str(fused),
                noise_mode=layer_kwargs.get('noise_mode', 'random'), use_noise=bool(block.conv1.use_noise), activation=block.conv1.activation,
                has_img=img is not None, split_ok=bool(_split_ok), x_dead=bool(_x_dead))])
            if tracer.skip_image is not None and block is tracer.skip_image[0]:
                img = tracer.skip_image[1](img)
            return real_forward(block, x, img, ws, force_fp32=force_fp32, fused_modconv=fused_modconv, update_emas=update_emas, _split_ok=_split_ok, _x_dead=_x_dead,
                                **layer_kwargs)
        cls.forward = forward
        return self

    def __exit__(self, *exc):
        from pix2pix3d_amd import _lib
        from pix2pix3d_amd.torch_utils.ops import modconv
        from pix2pix3d_amd.training import networks_stylegan2 as ns
        _lib._guarded = self._guarded
        torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream = self._waits
        for name, real in self._wrappers.items():
            setattr(modconv, name, real)
        modconv.SplitActs.__init__ = self._split_init
        if self._own_forward is None:
            del ns.SynthesisBlock.forward
        else:
            ns.SynthesisBlock.forward = self._own_forward


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


# ---- the recorded cases -------------------------------------------------------------------------------------------------------------------------------------------

SWITCHES = ('split_activations', 'split_bf16', 'fuse_torgb', 'fuse_torgb_256', 'fuse_wide_torgb', 'fuse_conv_wide_torgb', 'premodulate_rgb', 'sr_prefetch_ahead',
            'prefetch_styles', 'shared_weight_max_pixels')
HOOKS = ('last_backbone_conv1', 'middle_backbone_block', 'head_block1_conv1')
SKIP_IMAGES = ('strided', 'offset4')
MODELS = {'seg2cat': 'model_seg2cat', 'edge2car': 'model_edge2car', 'seg2face': 'model_full_seg2face_96'}      # name -> the golden whose latents and uniforms are replayed


def cases():
    """id -> dict(model, batch, force_fp32, noise_mode, and at most one of switch / hook / skip_image)."""
    out = {}
    for model in ('seg2cat', 'edge2car'):
        for batch in (1, 2, 4):
            for force_fp32 in (False, True):
                for noise_mode in ('const', 'none'):
                    out[f'{model}-b{batch}-{"fp32" if force_fp32 else "default"}-{noise_mode}'] = dict(model=model, batch=batch, force_fp32=force_fp32, noise_mode=noise_mode)
    # (an extra: build_generator offers seg2face with the full-size golden only — 128^2 rays, seconds per pass — so it is not run through the grid above)
    for force_fp32 in (False, True):
        out[f'seg2face-b2-{"fp32" if force_fp32 else "default"}-const'] = dict(model='seg2face', batch=2, force_fp32=force_fp32, noise_mode='const')
    base = dict(model='seg2cat', batch=4, force_fp32=False)
    out['seg2cat-b4-default-random'] = dict(base, noise_mode='random')
    for name in SWITCHES:
        out[f'seg2cat-b4-switch-{name}'] = dict(base, noise_mode='const', switch=name)
    for name in HOOKS:
        out[f'seg2cat-b4-hook-{name}'] = dict(base, noise_mode='const', hook=name)
    for name in SKIP_IMAGES:
        out[f'seg2cat-b4-skip-image-{name}'] = dict(base, noise_mode='const', skip_image=name)
    return out


def _strided(img):
    """The same image, dense in neither layout (a crop of a wider channels-last one)."""
    n, c, h, w = img.shape
    wide = torch.empty([n, c, h, w + 1], dtype=img.dtype, device=img.device).contiguous(memory_format=torch.channels_last)
    view = wide[..., :w]
    view.copy_(img)
    assert not view.is_contiguous() and not view.is_contiguous(memory_format=torch.channels_last)
    return view


def _offset4(img):
    """The same image, channels-last and dense, four bytes past a 16-byte boundary."""
    n, c, h, w = img.shape
    flat = torch.empty([img.numel() + 1], dtype=img.dtype, device=img.device)
    view = flat[1:].view(n, h, w, c).permute(0, 3, 1, 2)
    view.copy_(img)
    assert view.is_contiguous(memory_format=torch.channels_last) and view.data_ptr() % 16 == 4
    return view


def run_case(case):
    """One warm-up pass, then two traced ones: (the second's events, [digests of the first, of the second])."""
    from model_cases import build_generator, uniforms, replay_uniforms
    from conftest import load_golden
    from pix2pix3d_amd.torch_utils.ops import modconv
    from pix2pix3d_amd.training.superresolution import _SuperresolutionBase
    g = load_golden(MODELS[case['model']])
    G = build_generator(case['model'], 'cuda', **({'depth': tuple(int(v) for v in g['depth'])} if 'depth' in g.files else {}))
    n, nrr = case['batch'], int(g['nrr'])
    rows = [k % len(g['ws']) for k in range(n)]
    ws, c = torch.tensor(g['ws'][rows], device='cuda'), torch.tensor(g['c'][rows], device='cuda')
    u_c, u_f = uniforms(g, len(g['ws']), nrr, G.rendering_kwargs)      # (the golden's own draws, tiled over the batch like its latents)
    u_c, u_f = u_c[rows].cuda(), u_f.reshape(len(g['ws']), nrr * nrr, -1)[rows].reshape(n * nrr * nrr, -1).cuda()
    backbone = G.backbone.synthesis
    blocks = [getattr(backbone, f'b{res}') for res in backbone.block_resolutions]
    heads = [m for m in G.children() if isinstance(m, _SuperresolutionBase)]
    saved, handle, skip_image = None, None, None
    if 'switch' in case:
        saved = getattr(modconv, case['switch'])
        setattr(modconv, case['switch'], 0 if case['switch'] == 'shared_weight_max_pixels' else not saved)
    if 'hook' in case:
        target = {'last_backbone_conv1': blocks[-1].conv1, 'middle_backbone_block': blocks[len(blocks) // 2], 'head_block1_conv1': heads[0].block1.conv1}[case['hook']]
        handle = target.register_forward_hook(lambda module, args, output: None)
    if 'skip_image' in case:
        skip_image = (blocks[-1], {'strided': _strided, 'offset4': _offset4}[case['skip_image']])

    def once():
        torch.manual_seed(0)
        with Tracer(skip_image) as t, replay_uniforms(u_c, u_f), torch.no_grad():
            out = G.synthesis(ws, c, neural_rendering_resolution=nrr, noise_mode=case['noise_mode'], force_fp32=case['force_fp32'])
        torch.cuda.synchronize()
        return t.events, {k: digest(out[k]) for k in OUTPUTS}
    try:
        once()
        (_, first), (events, second) = once(), once()
    finally:
        if saved is not None:
            setattr(modconv, case['switch'], saved)
        if handle is not None:
            handle.remove()
    return json.loads(json.dumps(events)), [first, second]


def load_recording():
    with open(GOLDEN_FILE) as f:
        rec = json.load(f)
    return rec


def recorded_events(rec, case_id):
    return [rec['records'][k] for k in rec['cases'][case_id]['trace']]
