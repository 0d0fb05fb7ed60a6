"""renderer.render_route, the fallback guard, the descriptor builder and the draw replay, against the answers the code gave BEFORE the renderer's host path
had one route decision and one operand builder.

tests/golden/render_routes.npz was recorded from the commit before this refactor (b728407) by tests/golden/make_render_routes_golden.py, which drove that
commit's ``ImportanceRenderer.forward`` / ``run_model``, ``ImportanceSemanticRenderer.forward`` / ``run_model`` and ``shape._lattice_reason`` /
``_fallback_guard`` on the stand-ins and decoders below (``cases`` / ``facts`` are shared with that script, the answers are not) and stored, per case, four
small integers: ``KIND``, the reason class (``reason_class`` of that commit's text), ``PLANES`` and ``GUARD``.  Every case of the product of ``ENTRY_AXES`` is
there; none is filtered.  It also holds the bytes of the ``p3d_render_desc`` that commit's two builders filled for every launch (``desc_scenarios``).

One parent spelling became two: the two-plane-set renderer reported ``density_noise`` and ``clamp_mode`` as one condition (class 9); it now reports whichever
fails first, in the single-set renderer's order (5, then 6)."""
import collections
import ctypes
import itertools
import re
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden

POLICY = ['auto', 'require', 'never']
KIND = ['fused', 'fused_autograd', 'tensor_ops']
PLANES = ['in_place', 'expanded', 'ValueError']
GUARD = ['silent', 'warns', 'raises']
# reason classes: the first entry whose every key occurs in the text (both the parent's spellings and this tree's)
REASON_KEYS = [None, ('fused_policy',), ('CPU tensors',), ('autograd graph',), ('[N,3,32,H,W]',), ('density_noise > 0',), ("clamp_mode != 'softplus'",),
               ('decoder', ' not '), ('sample counts',), ('density_noise / clamp_mode',), ('sample_mixed',), ('renderer', ' not ')]
SAMPLES = [(3, 48), (4, 1), (48, 48), (64, 64), (65, 48), (48, 0), (48, 65)]
BATCHES = [(2, 2), (1, 3), (2, 3)]                                    # (plane batch, ray batch)
AXES = dict(policy=3, device=2, grad=2, fused_training=2, coords_grad=2, planes=3, dual_planes=4, batches=3, noise=2, clamp=2, samples=7, decoder=7,
            dual_decoder=2, generator=3)
_COMMON = ['policy', 'device', 'grad', 'fused_training']
ENTRY_AXES = {
    'forward': _COMMON + ['planes', 'batches', 'noise', 'clamp', 'samples', 'decoder'],
    'run_model': _COMMON + ['coords_grad', 'planes', 'batches', 'noise', 'clamp', 'decoder'],
    'dual_forward': _COMMON + ['dual_planes', 'batches', 'noise', 'clamp', 'samples', 'dual_decoder'],
    'dual_run_model': _COMMON + ['coords_grad', 'dual_planes', 'batches', 'noise', 'clamp', 'dual_decoder'],
    'sigma_grid': ['policy', 'device', 'generator', 'noise', 'decoder'],
}


def reason_class(text):
    if text is None:
        return 0
    for i in (9, 1, 2, 3, 4, 5, 6, 8, 10, 11, 7):
        if all(k in text for k in REASON_KEYS[i]):
            return i
    raise AssertionError(f'unclassified reason {text!r}')


class T:
    """Stand-in for a tensor: shape, device, requires_grad; ``expand`` marks the copy."""

    def __init__(self, shape, on_device, requires_grad=False, expanded=False):
        self.shape, self.ndim, self.requires_grad, self.expanded = torch.Size(shape), len(shape), requires_grad, expanded
        self.device, self.is_cuda = torch.device('cuda' if on_device else 'cpu'), on_device

    def expand(self, n, *rest):
        return T([n] + list(self.shape[1:]), self.is_cuda, self.requires_grad, True)


def cases(entry):
    names = ENTRY_AXES[entry]
    return [dict(zip(names, idx)) for idx in itertools.product(*[range(AXES[a]) for a in names])]


_decoders = {}


def decoders():
    """The decoder axes (built once; no parameter requires grad, so the ``grad`` axis alone decides whether a graph is needed)."""
    if not _decoders:
        from pix2pix3d_amd.training import triplane, triplane_cond as tc
        opt = lambda lr, **kw: dict(decoder_lr_mul=lr, decoder_output_dim=32, **kw)
        altered = triplane.OSGDecoder(32, opt(1))
        altered.net[2].weight_gain *= 2
        _decoders['decoder'] = [triplane.OSGDecoder(32, opt(1)), triplane.OSGDecoder(32, opt(0.5)), tc.OSGDecoder_semantic_lateSeparate(32, opt(1, sigmoid=False)),
                                tc.OSGDecoder_semantic(32, opt(1, sigmoid=False)), tc.OSGDecoder_semantic_entangle(32, opt(1, sigmoid=False, semantic_channels=6)),
                                altered, torch.nn.Linear(32, 33)]
        _decoders['dual_decoder'] = [(triplane.OSGDecoder(64, opt(1)), tc.OSGDecoder_semantic(32, opt(1, sigmoid=True))),
                                     (triplane.OSGDecoder(64, opt(1)), tc.OSGDecoder_semantic(32, opt(0.5, sigmoid=False)))]
        for group in _decoders.values():
            for d in group:
                for m in (d if isinstance(d, tuple) else (d,)):
                    m.requires_grad_(False)
    return _decoders


def facts(entry, c):
    """One case as the things an entry point is handed: stand-in tensors, options, decoder(s)."""
    on_device, grad = bool(c['device']), bool(c.get('grad', 0))
    nb, nr = BATCHES[c['batches']] if 'batches' in c else (2, 2)
    if 'dual_planes' in c:
        shapes = [([nb, 3, 32, 8, 8],) * 2, ([nb, 3, 16, 8, 8],) * 2, ([nb, 96, 8, 8],) * 2, ([nb, 3, 32, 8, 8], [nb, 3, 32, 4, 4])][c['dual_planes']]
    else:
        shapes = [([nb, 3, 32, 8, 8],), ([nb, 3, 16, 8, 8],), ([nb, 96, 8, 8],)][c.get('planes', 0)]
    sc, sf = SAMPLES[c['samples']] if 'samples' in c else (48, 48)
    options = dict(density_noise=[0, 0.1][c['noise']], clamp_mode=['softplus', 'relu'][c.get('clamp', 0)], depth_resolution=sc, depth_resolution_importance=sf,
                   ray_start=2.25, ray_end=3.3, box_warp=1.0, disparity_space_sampling=False, white_back=False)
    key = 'dual_decoder' if 'dual_decoder' in c else 'decoder'
    dec = decoders()[key][c[key]]
    return SimpleNamespace(policy=POLICY[c['policy']], on_device=on_device, grad=grad, fused_training=bool(c.get('fused_training', 1)),
                           coords_grad=bool(c.get('coords_grad', 0)), planes=[T(s, on_device, grad) for s in shapes], n_rays=nr, options=options,
                           decoders=dec if isinstance(dec, tuple) else (dec,), rays=T([nr, 16, 3], on_device), coords=T([nr, 16, 3], on_device, bool(c.get('coords_grad', 0))))


def generator(kind, decoder, options):
    """sigma_grid's generator axis: the tri-plane core as it is, one that overrides ``sample_mixed``, one with the two-plane-set renderer."""
    from pix2pix3d_amd.training.triplane import _TriPlaneCore
    from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod

    class Core(_TriPlaneCore):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.renderer = rmod.ImportanceSemanticRenderer() if kind == 2 else rmod.ImportanceRenderer()
            self.decoder, self.rendering_kwargs = decoder, options

    class Own(Core):
        def sample_mixed(self, *a, **k):
            raise NotImplementedError
    return (Own if kind == 1 else Core)()


def guard_outcome(call):
    """0 / 1 / 2: what a guard call does (``GUARD``)."""
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        try:
            call()
        except RuntimeError:
            return 2
    return 1 if seen else 0


@pytest.fixture
def switches():
    from pix2pix3d_amd import shape
    from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod
    saved = rmod.fused_policy, rmod.fused_training, set(rmod._warned_routes)
    yield rmod, shape
    rmod.fused_policy, rmod.fused_training = saved[:2]
    rmod._warned_routes.clear()
    rmod._warned_routes.update(saved[2])


@pytest.mark.parametrize('entry', ['forward', 'run_model', 'dual_forward', 'dual_run_model'])
def test_render_route_gives_the_answers_of_the_parents_two_route_decisions(entry, switches):
    rmod, _ = switches
    g = load_golden('render_routes')
    cs, answers = cases(entry), g[entry + '_answers'].tolist()
    assert len(cs) == len(answers) == int(g[entry + '_count']) and np.array_equal(g[entry + '_cases'], [list(c.values()) for c in cs])
    seen = collections.Counter()
    for c, (kind, reason, planes, guard) in zip(cs, answers):
        f = facts(entry, c)
        rmod.fused_policy = f.policy
        needs_grad = f.grad or f.coords_grad                      # (grad mode is on; rays and decoder parameters do not require grad)
        has_backward = {'forward': f.fused_training, 'run_model': f.fused_training and not f.coords_grad}.get(entry, False)
        try:
            r = rmod.render_route(entry, f.policy, f.on_device, needs_grad, has_backward, [p.shape for p in f.planes], f.n_rays, f.options, f.decoders)
        except ValueError as e:
            assert PLANES[planes] == 'ValueError' and re.search('batch %d .* batch %d' % BATCHES[c['batches']], str(e)), c
            seen['ValueError'] += 1
            continue
        want = 5 + (f.options['density_noise'] <= 0) if reason == 9 else reason
        assert (r.kind, reason_class(r.reason), PLANES[int(r.expand)]) == (KIND[kind], want, PLANES[planes]), (c, r)
        assert (r.reason is None) == (r.kind != 'tensor_ops'), c
        rmod._warned_routes.clear()
        got = 0 if r.reason is None else guard_outcome(lambda: rmod._tensor_op_guard('ImportanceRenderer', f.on_device, r.reason))
        assert got == guard, (c, r)
        seen[r.kind, want, r.expand, got] += 1
    assert bool(seen['ValueError']) == entry.endswith('forward') and all(      # (point queries take the planes' batch as it comes, as they did)
        seen[k, 0, False, 0] for k in KIND[:1 if entry.startswith('dual') else 2]) and len(seen) > 12, seen


def test_sigma_grid_falls_back_for_the_parents_reasons(switches):
    rmod, shape = switches
    g = load_golden('render_routes')
    cs, answers = cases('sigma_grid'), g['sigma_grid_answers'].tolist()
    assert len(cs) == len(answers) == int(g['sigma_grid_count']) and np.array_equal(g['sigma_grid_cases'], [list(c.values()) for c in cs])
    for c, (kind, reason, _, guard) in zip(cs, answers):
        f = facts('sigma_grid', c)
        rmod.fused_policy = f.policy
        G, ws = generator(c['generator'], f.decoders[0], f.options), T([1, 14, 512], f.on_device)
        text = shape._lattice_reason(G, ws)
        assert reason_class(text) == reason and (text is None) == (KIND[kind] == 'fused'), (c, text)
        rmod._warned_routes.clear()
        assert (0 if text is None else guard_outcome(lambda: shape._fallback_guard(ws, text))) == guard, (c, text)
    rmod.fused_policy = 'require'
    with pytest.raises(RuntimeError, match='lattice kernel required'):
        shape._fallback_guard(T([1, 14, 512], True), 'density_noise > 0')


def test_the_guard_warns_once_per_reason(switches):
    rmod, _ = switches
    rmod.fused_policy = 'auto'
    rmod._warned_routes.clear()
    call = lambda reason: guard_outcome(lambda: rmod._tensor_op_guard('ImportanceRenderer', True, reason))
    assert [call('density_noise > 0'), call('density_noise > 0'), call('CPU tensors')] == [1, 0, 1]


# ---- descriptors ----------------------------------------------------------------------------------------------------------------
class FakeLib:
    """Stands in for the kernel library on CPU tensors: every entry point succeeds, the descriptors it was handed are kept."""

    def __init__(self):
        self.descs = []

    def __getattr__(self, name):
        def fn(*args):
            self.descs += [bytes(a._obj) for a in args if hasattr(a, '_obj')]
            return 2 * 4257 if name == 'p3d_render_grad_decoder_floats' else 0
        return fn


def _plane_set(n, layout, seed):
    g = torch.Generator().manual_seed(seed)
    if layout == 'in_place':                                   # a channels-last [N,96,H,W] backbone output viewed as [N,3,32,H,W]
        return torch.randn(n, 8, 8, 96, generator=g).as_strided((n, 3, 32, 8, 8), (8 * 8 * 96, 32, 1, 8 * 96, 96))
    return torch.randn(n, 3, 32, 8, 8, generator=g)


def desc_scenarios(rmod, launch):
    """name -> the descriptor bytes of every launch; ``launch(kind, lib, ...)`` is the one place the parent's recorder and this test differ (the parent has no
    ``fused_render_dual`` / ``fused_sample_points_dual``: its recorder goes through ``_dual_operands``)."""
    from pix2pix3d_amd import _lib
    from pix2pix3d_amd.torch_utils.ops import modconv
    from pix2pix3d_amd.training import triplane, triplane_cond as tc
    dopt = lambda **kw: dict(decoder_lr_mul=1, decoder_output_dim=32, **kw)
    singles = {'osg': triplane.OSGDecoder(32, dopt()), 'late': tc.OSGDecoder_semantic_lateSeparate(32, dopt(sigmoid=True))}
    duals = {s: (triplane.OSGDecoder(64, dopt()), tc.OSGDecoder_semantic(32, dopt(sigmoid=s))) for s in (False, True)}
    m, sc, sf = 16, 6, 5
    out = {}
    saved = _lib.lib, _lib.stream_of, rmod.mlp_bf16x3, rmod.mlp_l1x6, modconv.f32_x6
    _lib.stream_of = lambda t: None
    try:
        for layout, limits, nb, nr in itertools.product(('in_place', 'default'), ('numeric', 'tensor'), (1, 3), (3,)):
            opt = dict(depth_resolution=sc, depth_resolution_importance=sf, ray_start=2.25, ray_end=3.3, box_warp=1.5, disparity_space_sampling=layout == 'default',
                       white_back=limits == 'tensor')
            ro, rd = torch.zeros(nr, m, 3), torch.ones(nr, m, 3)
            u_c, u_f = torch.zeros(nr, m, sc, 1), torch.zeros(nr * m, sf)
            t = (torch.zeros(nr, m, 1), torch.ones(nr, m, 1)) if limits == 'tensor' else (None, None)
            planes = _plane_set(nb, layout, 0)

            def record(name, kind, *args, **kw):
                lib = FakeLib()
                _lib.lib = lambda: lib
                launch(kind, *args, **kw)
                assert len(lib.descs) == 1, name
                out[f'{name}/{layout}/{limits}/planes{nb}'] = lib.descs[0]
            for dname, dec in singles.items():
                for mode in (0, 1, 2):
                    rmod.mlp_bf16x3, rmod.mlp_l1x6, modconv.f32_x6 = mode == 1, mode == 2, True
                    record(f'forward_{dname}_mode{mode}', 'forward', planes, dec, ro, rd, opt, u_c, u_f, *t)
                if nb == nr:
                    record(f'backward_{dname}', 'backward', planes, dec, ro, rd, opt, u_c, u_f, *t, torch.zeros(nr, m, 32 * (1 + (dname == 'late'))))
                if limits == 'numeric':
                    record(f'points_{dname}', 'points', planes, dec, torch.zeros(nb, 7, 3), opt)
                    record(f'lattice_{dname}', 'lattice', planes, dec, torch.zeros(4), torch.zeros(5), torch.zeros(6), opt)
            if nb == nr:
                sets = {'': (planes, _plane_set(nb, layout, 1)), '_odd': (planes, _plane_set(nb, 'default' if layout == 'in_place' else 'in_place', 1))}
                for sname, (pt, ps) in sets.items():
                    for sig, (dt, ds) in duals.items():
                        record(f'dual_forward{sname}_sigmoid{int(sig)}', 'dual_forward', pt, ps, dt, ds, ro, rd, opt, u_c, u_f, *t)
                        if limits == 'numeric':
                            record(f'dual_points{sname}_sigmoid{int(sig)}', 'dual_points', pt, ps, dt, ds, torch.zeros(nb, 7, 3), opt)
    finally:
        _lib.lib, _lib.stream_of, rmod.mlp_bf16x3, rmod.mlp_l1x6, modconv.f32_x6 = saved
    return out


def test_every_launch_gets_the_descriptor_the_parents_two_builders_gave_it():
    from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod
    fns = {'forward': rmod.fused_render, 'backward': rmod.fused_render_backward, 'points': rmod.fused_sample_points, 'lattice': rmod.fused_sample_lattice,
           'dual_forward': rmod.fused_render_dual, 'dual_points': rmod.fused_sample_points_dual}
    got = desc_scenarios(rmod, lambda kind, *a, **k: fns[kind](*a, **k))
    g = load_golden('render_routes')
    want = dict(zip(g['desc_names'].tolist(), g['desc_bytes']))
    assert sorted(got) == sorted(want) and len(got) >= 90
    fields = [f for f, _ in rmod._RenderDesc._fields_]
    for name, raw in want.items():
        a, b = rmod._RenderDesc.from_buffer_copy(got[name]), rmod._RenderDesc.from_buffer_copy(raw.tobytes())
        assert {f: getattr(a, f) for f in fields} == {f: getattr(b, f) for f in fields}, name
    # what must survive, spelled out (independently of the recording)
    d = lambda name: rmod._RenderDesc.from_buffer_copy(got[name])
    for name in got:
        kind, x = name.split('/')[0], d(name)
        if kind.startswith('dual'):
            assert (x.raster_order, x.mlp_bf16x3, x.n_nets, x.semantic_sigmoid) == (1, 0, 2, int(kind[-1])), name
        elif kind.startswith(('points', 'lattice')):
            assert (x.raster_order, x.mlp_bf16x3, x.rays_per_img) == (0, 0, 1), name
        elif kind.startswith('forward'):
            assert (x.raster_order, x.n_img, x.mlp_bf16x3) == (3 if name.endswith('planes1') else 1, 3, int(kind[-1])), name
        assert (x.image_stride, x.plane_stride, x.pixel_stride) == ((8 * 8 * 96, 32, 96) if '/in_place/' in name and '_odd' not in kind else (0, 0, 0)), name
        assert (x.ray_start, x.ray_end) == ((0.0, 0.0) if '/tensor/' in name or x.rays_per_img == 1 else (2.25, ctypes.c_float(3.3).value)), name


def test_desc_is_a_pure_function():
    from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod
    opt = dict(depth_resolution=48, depth_resolution_importance=32, box_warp=1.0, ray_start=2.25, ray_end=3.3, white_back=True)
    d = rmod.render_desc(4, 256, 16, 24, (6144, 32, 96), 2, True, 2, opt, numeric_limits=True, raster=3)
    assert [getattr(d, f) for f, _ in rmod._RenderDesc._fields_] == [4, 256, 16, 24, 2, 1, 48, 32, 0, 1, 2.25, ctypes.c_float(3.3).value, 1.0, 6144, 32, 96, 3, 2]


# ---- draws ----------------------------------------------------------------------------------------------------------------------
def test_replay_draws_hands_a_logical_draw_back_in_the_order_it_is_asked_for():
    from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod
    n, m, sc, sf = 3, 5, 4, 2
    u_c, u_f = torch.rand(n, m, sc, 1), torch.rand(n * m, sf)
    real = torch.rand, torch.rand_like
    with rmod._replay_draws(u_c, u_f):
        a, b = torch.rand([sc, n, m, 1], dtype=torch.float32), torch.rand(n * m, sf)
    assert a.data_ptr() == u_c.data_ptr() and a.stride() == u_c.permute(2, 0, 1, 3).stride() and torch.equal(a.permute(1, 2, 0, 3), u_c) and b.data_ptr() == u_f.data_ptr()
    with rmod._replay_draws(u_c, u_f):
        a, b = torch.rand([n, m, sc, 1]), torch.rand([n * m, sf])
    assert torch.equal(a, u_c) and a.data_ptr() == u_c.data_ptr() and torch.equal(b, u_f)
    with rmod._replay_draws(u_c, u_f):
        a = torch.rand_like(torch.empty(sc, n, m, 1).permute(1, 2, 0, 3))
        assert torch.equal(a, u_c)
    assert (torch.rand, torch.rand_like) == real
    # the renderer's own draws, both branches: what a route launches with is the logical draw
    with rmod._replay_draws(u_c, u_f):
        a, b = rmod._draw_uniforms(n, m, sc, sf, 'cpu', tensor_limits=True)
    assert torch.equal(a, u_c) and torch.equal(b, u_f)
