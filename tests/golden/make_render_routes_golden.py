"""Records tests/golden/render_routes.npz.  Run ONCE, in a checkout of b728407 (the commit before the renderer's host path got one route decision), with
tests/test_render_routes.py of this tree beside it for the case lists and stand-ins:

    python tests/golden/make_render_routes_golden.py

It drives that commit's entry points as far as their route decision: the launches and the tensor-op formulations are replaced by markers, so what is
recorded is which of them the entry point reached, with which planes, and what its guard did on the way.  No GPU is needed."""
import ctypes
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_render_routes as C  # noqa: E402
from pix2pix3d_amd import _lib, shape  # noqa: E402
from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod  # noqa: E402


class Reached(Exception):
    pass


class _Axes:
    def to(self, device):
        return self


class _Proxy:
    """A CPU tensor that says it is on the device."""
    device = torch.device('cuda')

    def __init__(self, t):
        self._t = t

    def __getattr__(self, name):
        return getattr(self._t, name)


def _reach(kind):
    def fn(*a, **k):
        raise Reached(kind)
    return fn


def _observe(renderer, call, tensor_op_name):
    """(kind, reason class, planes, guard) of one call of the parent's entry point."""
    seen = {'reason': None, 'expanded': 0}
    guard = renderer._tensor_op_guard

    def guarded(planes, reason):
        seen['reason'], seen['expanded'] = reason, int(bool(getattr(planes, 'expanded', False)))
        guard(planes, reason)

    def tensor_ops(planes, *a, **k):
        seen['expanded'] = int(bool(getattr(planes, 'expanded', False)))
    fused = getattr(renderer, '_forward_fused', None)

    def forward_fused(planes, *a, **k):
        seen['expanded'] = int(bool(planes.expanded))
        return fused(planes, *a, **k)
    renderer._tensor_op_guard = guarded
    setattr(renderer, tensor_op_name, tensor_ops)
    renderer._forward_fused = forward_fused
    rmod._warned_routes.clear()
    kind = 2
    with warnings.catch_warnings(record=True) as warned:
        warnings.simplefilter('always')
        try:
            call()
            outcome = 1 if warned else 0
        except Reached as e:
            kind, outcome = C.KIND.index(str(e)), 0
            assert seen['reason'] is None and not warned
        except RuntimeError as e:
            assert 'required but unavailable' in str(e), e
            outcome = 2
        except ValueError as e:
            assert 'cannot serve' in str(e), e
            return 0, 0, 2, 0
    return kind, C.reason_class(seen['reason']), seen['expanded'], outcome


def record_routes(entry):
    dual = entry.startswith('dual')
    answers = []
    for c in C.cases(entry):
        f = C.facts(entry, c)
        rmod.fused_policy, rmod.fused_training = f.policy, f.fused_training
        R = rmod.ImportanceSemanticRenderer() if dual else rmod.ImportanceRenderer()
        R.plane_axes = _Axes()
        if dual:
            operands = R._dual_operands

            def dual_operands(*a):
                ops = operands(*a)
                if not isinstance(ops, str) and entry == 'dual_run_model':
                    raise Reached('fused')
                return ops
            R._dual_operands = dual_operands
        if entry.endswith('forward'):
            call = lambda: R.forward(*f.planes, *f.decoders, f.rays, f.rays, f.options)
            name = '_forward_tensor_ops'
        else:
            call = lambda: R.run_model(*f.planes, *f.decoders, f.coords, f.rays, f.options)
            name = '_run_model_tensor_ops' if dual else '_points_tensor_ops'
        answers.append(_observe(R, call, name))
    return answers


def record_sigma_grid():
    answers = []
    for c in C.cases('sigma_grid'):
        f = C.facts('sigma_grid', c)
        rmod.fused_policy = f.policy
        G, ws = C.generator(c['generator'], f.decoders[0], f.options), C.T([1, 14, 512], f.on_device)
        reason = shape._lattice_reason(G, ws)
        shape._warned.clear()
        guard = 0 if reason is None else C.guard_outcome(lambda: shape._fallback_guard(ws, reason))
        answers.append((0 if reason is None else 2, C.reason_class(reason), 0, guard))
    return answers


def parent_launch(kind, *args, **kw):
    if not kind.startswith('dual'):
        fns = {'forward': rmod.fused_render, 'backward': rmod.fused_render_backward, 'points': rmod.fused_sample_points, 'lattice': rmod.fused_sample_lattice}
        return fns[kind](*args, **kw)
    pt, ps, dt, ds = args[:4]
    opt = args[6] if kind == 'dual_forward' else args[5]
    ops = rmod.ImportanceSemanticRenderer()._dual_operands(_Proxy(pt), _Proxy(ps), dt, ds, opt, False)
    assert not isinstance(ops, str), ops
    desc = ops[3]
    if kind == 'dual_points':
        d = desc()                                             # as ImportanceSemanticRenderer.run_model calls it
    else:
        auto = args[9] is not None                             # ... and as forward does
        d = desc(args[4].shape[1], 0.0 if auto else opt['ray_start'], 0.0 if auto else opt['ray_end'])
    _lib.lib().p3d_record(ctypes.byref(d))


def main():
    real = torch.rand, torch.empty, rmod.fused_render, rmod.fused_sample_points, rmod._plane_set_cl, _lib.lib, _lib.stream_of
    out = {}
    try:
        # the two draws stand for "about to launch": the single-set renderer goes on to one of the two launchers, the two-plane-set renderer launches itself
        torch.rand = lambda *a, **k: real[0](1)
        rmod.fused_render, rmod._FusedRenderFn.apply = _reach('fused'), _reach('fused_autograd')
        rmod.fused_sample_points, rmod._FusedPointsFn.apply = _reach('fused'), _reach('fused_autograd')
        for entry in ('forward', 'run_model'):
            out[entry] = record_routes(entry)
        torch.rand = _reach('fused')
        torch.empty = lambda *a, **k: real[1](*a, **{**k, 'device': 'cpu'})
        rmod._plane_set_cl = lambda planes: (real[1](1), (0, 0, 0))
        fake = C.FakeLib()
        _lib.lib, _lib.stream_of = (lambda: fake), (lambda t: None)
        for entry in ('dual_forward', 'dual_run_model'):
            out[entry] = record_routes(entry)
        out['sigma_grid'] = record_sigma_grid()
    finally:
        torch.rand, _, rmod.fused_render, rmod.fused_sample_points, rmod._plane_set_cl, _lib.lib, _lib.stream_of = real
        del rmod._FusedRenderFn.apply, rmod._FusedPointsFn.apply
    rmod.fused_policy, rmod.fused_training = 'auto', True
    try:                                                       # (torch.empty still answers on the CPU for the proxies of the two-plane-set launches)
        descs = C.desc_scenarios(rmod, parent_launch)
    finally:
        torch.empty = real[1]
    arrays = {'desc_names': np.array(sorted(descs)), 'desc_bytes': np.array([np.frombuffer(descs[k], np.uint8) for k in sorted(descs)])}
    for entry, answers in out.items():
        cs = C.cases(entry)
        assert len(cs) == len(answers)
        arrays[entry + '_cases'] = np.array([list(c.values()) for c in cs], np.uint8)
        arrays[entry + '_answers'] = np.array(answers, np.uint8)
        arrays[entry + '_count'] = np.array(len(cs))
        print(entry, len(cs), np.unique(arrays[entry + '_answers'], axis=0, return_counts=True))
    print(len(descs), 'descriptors')
    np.savez_compressed(os.path.join(HERE, 'render_routes.npz'), **arrays)


if __name__ == '__main__':
    main()
