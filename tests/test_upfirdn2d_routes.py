"""The upfirdn2d case table (tests/upfirdn2d_routes.py) against the C++ dispatch it restates, and the float64 adjoint the GPU tests
compare gradients with.  No GPU needed."""
import numpy as np
import pytest
import torch

import upfirdn2d_routes as R
from oracle import ops_oracle as O


def test_restated_lists_are_the_dispatch_lists():
    tiled, cl, gen, fully_generic, fir4 = R.dispatch_lists()
    assert tiled == R.TILED and cl == R.CL and gen == R.GENERIC and fully_generic and fir4


def test_case_table_reaches_every_instantiation():
    """A new instantiation in csrc/upfirdn2d.hip fails here until a case reaches it: the tiled and channels-last routes in fp32 and
    fp16 (fir4's u = d = 1 cases count for upfirdn2d_cl_kernel<T, 1, 1, 4> too: the GPU test reruns them with P3D_UPFIRDN_NO_FIR4),
    accumulate mode in both, each generic specialisation in some dtype."""
    tiled, cl, gen, _, _ = R.dispatch_lists()
    reached = set()
    for c in R.CASES:
        for no_fir4 in (False, True):
            reached.update((r, c.dtype) for r in R.wrapper_routes(c, no_fir4=no_fir4))
    reached.update((R.acc_route(dt, shape), dt) for _, dt, shape in R.ACC_CASES)
    need = [(f'tiled<{u},{d},{f}>', dt) for u, d, f in tiled for dt in ('f32', 'f16')]
    need += [(f'cl<{u},{d},{f}>', dt) for u, d, f in cl for dt in ('f32', 'f16')]
    need += [('fir4', dt) for dt in ('f32', 'f16')] + [('cl<2,1,4>+acc', dt) for dt in ('f32', 'f16')]
    assert [k for k in need if k not in reached] == []
    routes = {r for r, _ in reached}
    assert [k for k in ['generic<%d,%d,%d,%d,%d,%d>' % g for g in gen] + ['generic<0,0,0,0,0,0>'] if k not in routes] == []
    assert routes <= set(R.all_routes())


def test_cases_take_their_declared_routes():
    for c in R.CASES:
        assert R.wrapper_routes(c) == c.routes, c.name
        assert len(R.grad_routes(c)) == len(c.routes), c.name
    names = [c.name for c in R.CASES]
    assert len(set(names)) == len(names)


def test_production_cases_come_from_the_model_config():
    """D's blocks at 512^2 / 256^2 are fp16 with 64 / 128 channels, the Encoder's fp32: each runs the fused 4-tap kernel in front of its
    stride-2 3 x 3 conv, and the channels-last down = 2 kernel in front of its 1 x 1 skip (whose gradient is the up = 2 one)."""
    cs = R.production_cases()
    assert [c.name for c in cs] == R.PRODUCTION
    for c in cs:
        assert R.wrapper_routes(c) == c.routes
        assert R.grad_routes(c) == (['fir4'] if c.routes == ['fir4'] else ['cl<2,1,4>'])
        assert c.shape[0] == 4 and c.shape[1] * c.shape[2] == 32768


def _small(c):
    return int(np.prod(c.shape)) <= 200000


@pytest.mark.parametrize('case', [c for c in R.CASES if _small(c)], ids=[c.name for c in R.CASES if _small(c)])
def test_oracle_adjoint_is_autograd_of_the_reference(case):
    """O.upfirdn2d_grad against float64 autograd through upfirdn2d(..., impl='ref') (the zero-stuff + pad + conv2d formulation), and
    O.upfirdn2d against that formulation's forward.  (impl='ref' rounds f * gain to fp32 before it casts the filter: 2e-7.)"""
    from pix2pix3d_amd.torch_utils.ops import upfirdn2d
    up, down, pad = R._geom(case)
    kw = dict(up=list(up), down=list(down), padding=list(pad), flip_filter=case.flip, gain=case.gain)
    g = torch.Generator().manual_seed(len(case.name))
    x = torch.randn(case.shape, generator=g, dtype=torch.float64, requires_grad=True)
    f = R.make_filter(case.filt, 3)
    y = upfirdn2d.upfirdn2d(x, None if f is None else torch.tensor(f), impl='ref', **kw)
    assert np.abs(y.detach().numpy() - O.upfirdn2d(x.detach().numpy(), f, **kw)).max() <= 2e-7 * max(np.abs(y.detach().numpy()).max(), 1)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    gx, = torch.autograd.grad(y, x, gy)
    gxo = O.upfirdn2d_grad(gy.numpy(), case.shape, f, **kw)
    assert np.abs(gx.numpy() - gxo).max() <= 2e-7 * max(np.abs(gxo).max(), 1)
